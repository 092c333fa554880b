"""The MRF patch-matching style loss (preset keys mrf_factor / mrf_stride / mrf_max_patches / mrf_layers) end to end on the GPU: optim + the
loss modules over the kernels of csrc/mrf.hip against the restatement of the whole network (tests/mrf_restatement.MrfNet).  Synthetic VGG-19
weights and images at 64 x 64, three style layers (64 x 64, 32 x 32 and 16 x 16 pixels); the term sits on relu3_1 (196 queries of 256
channels against the 49 patches of the style's 16 x 16 map at stride 2) unless a configuration says otherwise.

Bars (those of tests/test_feat_hist_style_gpu.py for the same comparison): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4.

The evaluation is compared with the restatement's under the SAME decisions.  The nearest patch of a query is a decision, and the loss's
gradient is not continuous across it; the fp32 network hands the term activations that differ from the fp64 network's in their last bits.
So the activations that reach the style modules are recorded during the evaluation (forward pre-hooks), the device's nn for them is read
back (the kernels give the same bits for the same input: tests/test_mrf_gpu.py) and the fp64 evaluation takes it as given - by the patch's
origin, not its index, so that the two banks need not list the same patches.  The test prints how many decisions the fp64 network would
take differently.  With hist_loss_factor > 0 the bins are pinned the same way (tests/test_feat_hist_style_gpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import feat_hist_restatement as hr
import mrf_restatement as mr
import synth
from conftest import PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4
LAYERS = "relu1_1,relu2_1,relu3_1"
REASON = "MRF patch-matching StyleLoss runs on the module path"

# configuration -> (restatement fields, preset keys, flags)
CONFIGS = {
    "relu3_1": (dict(mrf_factor=1.0, mrf_layers="relu3_1"), dict(mrf_factor=1.0, mrf_layers="relu3_1"), []),
    "stride1-two-layers": (dict(mrf_factor=0.5, mrf_stride=1, mrf_layers="relu2_1,relu3_1"),
                           dict(mrf_factor=0.5, mrf_stride=1, mrf_layers="relu2_1,relu3_1"), []),
    "capped": (dict(mrf_factor=1.0, mrf_stride=1, mrf_max_patches=30, mrf_layers="relu3_1"),
               dict(mrf_factor=1.0, mrf_stride=1, mrf_max_patches=30, mrf_layers="relu3_1"), []),
    "with-histograms": (dict(mrf_factor=1.0, mrf_layers="relu3_1", hist_loss_factor=0.5),
                        dict(mrf_factor=1.0, mrf_layers="relu3_1", hist_loss_factor=0.5), []),
    "with-mirrors-shift-covariance": (dict(mrf_factor=1.0, mrf_layers="relu3_1", flip_factor=0.5, shift_factor=0.5, use_covariance=True),
                                      dict(mrf_factor=1.0, mrf_layers="relu3_1", flip_factor=0.5), ["--shift_factor", "0.5", "--use_covariance"]),
}


def preset_args(tmp_path, weight_files, preset, extra=(), **kw):
    """The namespace a user gets from --load_args with the preset keys (there is no flag for them)."""
    path = tmp_path / "mrf.json"
    path.write_text(json.dumps(preset))
    return product_args(weight_files, ["--load_args", str(path), "--style_layers", LAYERS] + list(extra), **kw)


def prepared(args, content, styles, init, size):
    """The network as optim.optimize prepares it, and the optimiser that evaluates it."""
    import models
    import optim
    optim.set_model_args(args, size)
    net, losses = models.load_model(args)
    optim.set_content_targets(net, content, args)
    optim.set_style_targets(net, styles, args)
    for m in losses:
        m.mode = "loss"
    return net, losses, optim.PixelOptimizer(net, losses, init, args)


def device_decisions(m, act, ref_origin):
    """nn of the module's kernels for the recorded activation act (1, C, H, W), as indices into the restatement's bank."""
    import hip
    smap, origin, inv = m.mrf_bank
    _, state = hip.mrf_fwd(act.cuda().contiguous(), smap, origin, inv)
    nn = hip.mrf_state_parts(state, act.shape[2], act.shape[3])[0].cpu().long()
    where = {int(o): p for p, o in enumerate(ref_origin.tolist())}
    return torch.tensor([where[int(o)] for o in origin.cpu()[nn].tolist()])[None, :]


def check_evaluation(cfg, args, sd, content, styles, init, size):
    from oracle.style_oracle import loss_order
    ref = mr.build_net(content.double(), [s.double() for s in styles], cfg, sd)
    net, losses, opt = prepared(args, content, styles, init, size)
    seen = []  # the activations the style modules get in this evaluation, in network order
    hooks = [m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().cpu())) for m in net.style_losses]
    slots, total, grad = opt.feval()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert opt.engine is None
    style_slots = [k for k, l in enumerate(ref.spec) if l.kind == "style"]
    assert len(seen) == len(style_slots) and all(a.shape[0] == 1 for a in seen)
    with_term = [i for i, m in zip(style_slots, net.style_losses) if m.mrf_factor > 0]
    assert with_term == ref.mrf_slots and with_term
    nn = {}
    own = ref.mrf_nearest(init.double())
    for i, m, a in zip(style_slots, net.style_losses, seen):
        if i not in with_term:
            assert m.mrf_bank is None and m._mrf_maps == []
            continue
        s_r, origin_r, inv_r = ref.mrf_banks[i]
        assert rel_l2(m.mrf_bank[0].cpu(), s_r) <= 1e-5 and m.mrf_bank[1].numel() == origin_r.numel(), m.name
        nn[i] = device_decisions(m, a, origin_r)
        print(f"  {m.name}: {origin_r.numel()} patches, {nn[i].numel()} queries, {int((nn[i][0] != own[i]).sum())} decided differently by the fp64 network")
    pinned = {i: hr.decide(a[0], ref.bins)[2] for i, a in zip(style_slots, seen)} if ref.hist_loss_factor > 0 else None
    total_r, losses_r, grad_r = ref.feval(init.double(), pinned=pinned, nn=nn)
    order = loss_order(ref.spec)
    assert len(order) == len(losses)
    got = slots.cpu().double()
    for k, i in enumerate(order):
        want = float(losses_r[i]) if i in losses_r else 0.0
        print(f"  {losses[k].name}: {float(got[k]):.9e} (fp64 {want:.9e})")
        assert abs(float(got[k]) - want) <= TOL_LOSS * abs(want), (losses[k].name, float(got[k]), want)
    e = rel_l2(grad.cpu(), grad_r)
    print(f"  pixel gradient rel-L2 {e:.3e} (bar {TOL_GRAD:.1e})")
    assert abs(float(total) - float(total_r)) <= TOL_LOSS * abs(float(total_r))
    assert e <= TOL_GRAD
    return ref, net, opt


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vgg19_at_64(tmp_path, weight_files, name):
    over, preset, flags = CONFIGS[name]
    cfg = make_cfg(style_layers=LAYERS, **over)
    args = preset_args(tmp_path, weight_files, preset, flags, S=64)
    content, style, init = synth.images(64)
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 64)
    if name == "relu3_1":
        assert ref.mrf_banks[ref.mrf_slots[0]][1].numel() == 49  # the 16 x 16 map at stride 2
        # the term is there: the layer's slot is larger than without it, by factor x m x strength and what normalisation makes of it
        plain = mr.build_net(content.double(), [style.double()], make_cfg(style_layers=LAYERS), synth.vgg19_state_dict(dtype=torch.float64))
        i = ref.mrf_slots[0]
        assert float(ref.feval(init.double())[1][i]) > float(plain.feval(init.double())[1][i])
    if name == "capped":
        assert ref.mrf_banks[ref.mrf_slots[0]][1].numel() == 25  # 14 x 14 = 196 and 7 x 7 = 49 are over the cap of 30: stride 3, 5 x 5


def test_two_styles_of_different_sizes_share_one_bank(tmp_path, weight_files):
    over = dict(mrf_factor=1.0, mrf_stride=1, mrf_layers="relu3_1")
    cfg = make_cfg(style_layers=LAYERS, style_blend_weights=[0.25, 0.75], **over)
    args = preset_args(tmp_path, weight_files, over, ["--style_blend_weights", "0.3,0.9"], S=64, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content, _, init = synth.images(64)
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 90, 70, generator=gen) * 255 - 120
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, 64)
    m = net.style_losses[2]
    smap, origin, _ = m.mrf_bank
    (h1, w1), (h2, w2) = (tuple(a.shape[1:]) for a in m._mrf_maps)
    assert (h1, w1) != (h2, w2) and tuple(smap.shape[1:]) == (h1 + h2, max(w1, w2)) and origin.numel() <= (h1 - 2) * (w1 - 2) + (h2 - 2) * (w2 - 2)
    ys, xs = origin.cpu().long() // smap.shape[2], origin.cpu().long() % smap.shape[2]
    first = (ys + 2 < h1) & (xs + 2 < w1)
    second = (ys >= h1) & (xs + 2 < w2)
    assert bool((first ^ second).all()) and bool(first.any()) and bool(second.any())  # no patch across the two maps or in a map's padding
    assert not bool(smap[:, :h1, w1:].any()) and not bool(smap[:, h1:, w2:].any())


def test_factor_zero_gives_the_bits_of_a_run_without_the_keys(tmp_path, weight_files):
    content, style, init = synth.images(64)
    _, _, with_key = prepared(preset_args(tmp_path, weight_files, dict(mrf_factor=0, mrf_stride=1, mrf_layers="relu3_1"), S=64), content, [style], init, 64)
    _, _, without = prepared(product_args(weight_files, ["--style_layers", LAYERS], S=64), content, [style], init, 64)
    assert with_key.engine is not None and without.engine is not None  # both on the fused engine
    assert all(m.mrf_bank is None and m._mrf_maps == [] for m in with_key.net.style_losses)
    a, b = with_key.feval(), without.feval()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_two_frames_at_module_level_are_evaluated_per_frame():
    """B = 2, and a style clip of two frames: the bank holds both frames' patches, every working frame is matched on its own."""
    import hip
    import loss
    gen = torch.Generator().manual_seed(7)
    C, H, W, s, mf = 8, 13, 18, 3.0, 0.5
    style = torch.relu(torch.randn(2, C, H + 2, W + 1, generator=gen) + 0.3)
    x = torch.relu(torch.randn(2, C, H, W, generator=gen) + 0.3)
    m = loss.StyleLoss(s)
    m.name = "style_two_frames"
    m.mrf_factor, m.mrf_stride = mf, 1
    m.mode, m.blend_weight = "capture", 1.0
    m(style.cuda())
    assert len(m._mrf_maps) == 2
    m.mode = "loss"
    xg = x.cuda().requires_grad_(True)
    m(xg)
    m.loss.backward()
    s_r, origin_r, inv_r, _ = mr.build_bank([style[0], style[1]], 1, 16384)
    assert torch.equal(m.mrf_bank[0].cpu(), s_r) and torch.equal(m.mrf_bank[1].cpu(), origin_r) and origin_r.numel() == 2 * 13 * 17

    def gram(f):
        flat = f.reshape(C, -1)
        return flat @ flat.t() / f.nelement()

    s64 = style.double()
    g_target = (gram(s64[0]) + gram(s64[1])) / 2   # blend weight x G / frames, per frame
    x64 = x.double().requires_grad_(True)
    want = 0
    for b in range(2):
        _, state = hip.mrf_fwd(x[b].cuda(), *m.mrf_bank)
        nn = hip.mrf_state_parts(state, H, W)[0].cpu().long()
        d = mr.patches(x64[b]) - mr.bank_patches(s_r.double(), origin_r)[nn]
        want = want + (((gram(x64[b]) - g_target) ** 2).mean() + mf * d.pow(2).mean()) * s / 2
    want.backward()
    assert abs(float(m.loss.detach()) - float(want.detach())) <= TOL_LOSS * abs(float(want.detach()))
    assert rel_l2(xg.grad.cpu(), x64.grad) <= TOL_GRAD


@pytest.mark.parametrize("terms_engine", [0, 1])
def test_the_route_is_the_module_path_with_its_reason(tmp_path, weight_files, terms_engine):
    import engine
    import optim
    content, style, init = synth.images(64)
    preset = dict(mrf_factor=1.0, mrf_layers="relu3_1", terms_engine=terms_engine)
    net, losses, opt = prepared(preset_args(tmp_path, weight_files, preset, S=64), content, [style], init, 64)
    assert [m.mrf_factor for m in net.style_losses] == [0.0, 0.0, 1.0]
    assert opt.engine is None and optim._patch_matched(net) and optim._engine_of(net) is None
    assert optim._terms_on_module_path(net) == REASON and optim._terms_on_module_path(losses) == REASON
    opt.step()
    assert opt.engine is None
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        engine.StyleEngine(net, losses)
    for m in net.style_losses:  # back at 0 the same network takes the engine again
        m.mrf_factor = 0
    assert optim._terms_on_module_path(net) is None and not optim._style_targets_missing(net)
    back = optim.PixelOptimizer(net, losses, init, product_args(weight_files, ["--style_layers", LAYERS], S=64))
    assert back.engine is not None
    back.feval()
    net.style_losses[2].mrf_factor = 1.0  # switched on again behind the engine's back: it refuses the evaluation
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        back.engine.feval(back.x, capture=False)


def test_ten_lbfgs_iterations_lower_the_mrf_term(tmp_path, weight_files):
    import optim
    over = dict(mrf_factor=1.0, mrf_layers="relu3_1")
    cfg = make_cfg(style_layers=LAYERS, **over)
    args = preset_args(tmp_path, weight_files, over, S=64, N=10)
    content, style, init = synth.images(64)
    out = optim.optimize(content, [style], init.clone(), 10, args)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    ref = mr.build_net(content.double(), [style.double()], cfg, synth.vgg19_state_dict(dtype=torch.float64))
    before, after = ref.mrf_terms(init.double()), ref.mrf_terms(out.double())
    assert len(before) == 1
    for i in before:
        print(f"  style layer at {i}: m {before[i]:.6e} -> {after[i]:.6e}")
        assert after[i] < before[i], (i, before[i], after[i])
    assert rel_l2(out, init) > 1e-3  # (it moved)


def test_cli_with_the_preset_key(tmp_path, weight_files):
    """style.py --load_args mrf.json --image_sizes 64 --num_iters 5 finishes, and its picture differs from the run's without the preset."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    preset = tmp_path / "mrf.json"
    preset.write_text(json.dumps({"mrf_factor": 1.0}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    images = {}
    for label, extra in (("mrf", ["--load_args", str(preset)]), ("plain", [])):
        out = tmp_path / label
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), *extra,
                            "--image_sizes", "64", "--num_iters", "5", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                            str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out)], cwd=PKG,
                           env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_64.png"]
        images[label] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["mrf"].shape == (64, 64, 3)
    assert np.abs(images["mrf"] - images["plain"]).max() > 0
