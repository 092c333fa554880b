"""The feature-histogram style loss (preset keys hist_loss_factor / hist_loss_bins / hist_loss_knots) end to end on the GPU: optim + the loss
modules over the kernels of csrc/feat_hist.hip against the restatement (tests/feat_hist_restatement.py).  Synthetic VGG-19 weights and
images at 64 x 64, three style layers (64 x 64, 32 x 32 and 16 x 16 pixels).

Bars (those of tests/test_flip_style_gpu.py for the same comparison): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4.

The evaluation is compared with the restatement's under the SAME bin decisions.  The bin of an element is a decision, and the matched value
is not continuous across it (feat_hist_restatement.HistNet.feval says why: q jumps by up to 1 / N for the elements of two bins when one
element changes sides).  The kernels and the restatement take the same decisions on the same input - tests/test_feat_hist_gpu.py: the counts
are equal - but the fp32 network hands the term activations that differ from the fp64 network's in their last bits, and an element or two
of the three layers then falls on the other side of an edge (the test prints how many): measured on an MI355X with free decisions the pixel gradient is 3.1e-4 from the restatement's
with the default 256 bins and 5.2e-4 with 16, beside 3.6e-4 and 2.5e-5 for the restatement in fp32 against itself in fp64 - a property of
the definition, not of either implementation, and no bar below 1e-3 holds there.  So the activations that reach the style modules are
recorded during the evaluation (forward pre-hooks), their bins are decided by the restatement's own `decide`, and the fp64 evaluation takes
those bins as given (`pinned`) - what the oracle pinned to the engine's ReLU and pooling decisions (tests/engine_decisions.py) does for the network.  The bars
stay the fixed ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import feat_hist_restatement as hr
import synth
from conftest import PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4
LAYERS = "relu1_1,relu2_1,relu3_1"
REASON = "feature-histogram StyleLoss runs on the module path"

# configuration -> (restatement fields, preset keys, flags)
CONFIGS = {
    "defaults": (dict(hist_loss_factor=1.0), dict(hist_loss_factor=1.0), []),
    "bins16": (dict(hist_loss_factor=1.0, hist_loss_bins=16), dict(hist_loss_factor=1.0, hist_loss_bins=16), []),
    "bins64-knots128": (dict(hist_loss_factor=0.5, hist_loss_bins=64, hist_loss_knots=128), dict(hist_loss_factor=0.5, hist_loss_bins=64, hist_loss_knots=128), []),
    "with-mirrors-shift-covariance": (dict(hist_loss_factor=1.0, flip_factor=0.5, shift_factor=0.5, use_covariance=True),
                                      dict(hist_loss_factor=1.0, flip_factor=0.5), ["--shift_factor", "0.5", "--use_covariance"]),
}


def preset_args(tmp_path, weight_files, preset, extra=(), **kw):
    """The namespace a user gets from --load_args with the preset keys (there is no flag for them)."""
    path = tmp_path / "hist.json"
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


def check_evaluation(cfg, args, sd, content, styles, init, size):
    from oracle.style_oracle import loss_order
    ref = hr.build(content.double(), [s.double() for s in styles], cfg, sd)
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
    pinned = {i: hr.decide(a[0], ref.bins)[2] for i, a in zip(style_slots, seen)}
    total_r, losses_r, grad_r = ref.feval(init.double(), pinned=pinned)
    moved = {i: int((hr.decide(ref.net._forward(init.double())[0][i][0], ref.bins)[2] != pinned[i]).sum()) for i in style_slots}
    print(f"  elements whose bin the fp32 run and the fp64 network decide differently, per style layer: {moved}")
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


def check_targets(ref, net):
    slots = [k for k, l in enumerate(ref.spec) if l.kind == "style"]
    assert len(slots) == len(net.style_losses) == 3
    for i, m in zip(slots, net.style_losses):
        assert tuple(m.hist_target.shape) == tuple(ref.hist_targets[i].shape) == (m.target.shape[0], ref.knots)
        assert rel_l2(m.hist_target.cpu(), ref.hist_targets[i]) <= 1e-5, m.name
        assert bool((m.hist_target[:, 1:] >= m.hist_target[:, :-1]).all())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vgg19_at_64(tmp_path, weight_files, name):
    over, preset, flags = CONFIGS[name]
    cfg = make_cfg(style_layers=LAYERS, **over)
    args = preset_args(tmp_path, weight_files, preset, flags, S=64)
    content, style, init = synth.images(64)
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 64)
    check_targets(ref, net)


def test_two_styles_of_different_sizes_with_blend_weights(tmp_path, weight_files):
    cfg = make_cfg(style_layers=LAYERS, style_blend_weights=[0.25, 0.75], hist_loss_factor=1.0)
    args = preset_args(tmp_path, weight_files, dict(hist_loss_factor=1.0), ["--style_blend_weights", "0.3,0.9"], S=64, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content, _, init = synth.images(64)
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 90, 70, generator=gen) * 255 - 120
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, 64)
    check_targets(ref, net)


def test_factor_zero_gives_the_bits_of_a_run_without_the_key(tmp_path, weight_files):
    content, style, init = synth.images(64)
    _, _, with_key = prepared(preset_args(tmp_path, weight_files, dict(hist_loss_factor=0, hist_loss_bins=64), S=64), content, [style], init, 64)
    _, _, without = prepared(product_args(weight_files, ["--style_layers", LAYERS], S=64), content, [style], init, 64)
    assert with_key.engine is not None and without.engine is not None  # both on the fused engine
    assert all(m.hist_target is None for m in with_key.net.style_losses)
    a, b = with_key.feval(), without.feval()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_two_frames_at_module_level_are_evaluated_per_frame():
    import loss
    gen = torch.Generator().manual_seed(7)
    C, H, W, s, hf, bins, knots = 8, 13, 18, 3.0, 0.5, 64, 32
    style = torch.relu(2 * torch.randn(2, C, H + 2, W + 1, generator=gen) + 1)
    x = torch.relu(torch.randn(2, C, H, W, generator=gen) + 0.3)
    m = loss.StyleLoss(s)
    m.name = "style_two_frames"
    m.hist_loss_factor, m.hist_loss_bins, m.hist_loss_knots = hf, bins, knots
    m.mode, m.blend_weight = "capture", 1.0
    m(style.cuda())
    assert tuple(m.hist_target.shape) == (C, knots)
    m.mode = "loss"
    xg = x.cuda().requires_grad_(True)
    m(xg)
    m.loss.backward()

    def gram(f):
        flat = f.reshape(C, -1)
        return flat @ flat.t() / f.nelement()

    s64 = style.double()
    g_target = (gram(s64[0]) + gram(s64[1])) / 2   # blend weight x G / frames, per frame
    h_target = (hr.quantile_table(s64[0], knots) + hr.quantile_table(s64[1], knots)) / 2
    assert rel_l2(m.hist_target.cpu(), h_target) <= 1e-6
    x64 = x.double().requires_grad_(True)
    want = 0
    for b in range(2):
        want = want + (((gram(x64[b]) - g_target) ** 2).mean() + hf * hr.term(x64[b], h_target, bins)) * s / 2
    want.backward()
    assert abs(float(m.loss.detach()) - float(want.detach())) <= TOL_LOSS * abs(float(want.detach()))
    assert rel_l2(xg.grad.cpu(), x64.grad) <= TOL_GRAD


@pytest.mark.parametrize("terms_engine", [0, 1])
def test_the_route_is_the_module_path_with_its_reason(tmp_path, weight_files, terms_engine):
    import engine
    import optim
    content, style, init = synth.images(64)
    preset = dict(hist_loss_factor=1.0, terms_engine=terms_engine)
    net, losses, opt = prepared(preset_args(tmp_path, weight_files, preset, S=64), content, [style], init, 64)
    assert all(bool(m.terms_engine) == bool(terms_engine) for m in net.style_losses)
    assert opt.engine is None and optim._histogrammed(net) and optim._engine_of(net) is None
    assert optim._terms_on_module_path(net) == REASON and optim._terms_on_module_path(losses) == REASON
    opt.step()
    assert opt.engine is None
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        engine.StyleEngine(net, losses)
    for m in net.style_losses:  # back at 0 the same network takes the engine again
        m.hist_loss_factor = 0
    assert optim._terms_on_module_path(net) is None and not optim._style_targets_missing(net)
    back = optim.PixelOptimizer(net, losses, init, product_args(weight_files, ["--style_layers", LAYERS], S=64))
    assert back.engine is not None
    back.feval()
    net.style_losses[0].hist_loss_factor = 1.0  # switched on again behind the engine's back: it refuses the evaluation
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        back.engine.feval(back.x, capture=False)


def test_ten_lbfgs_iterations_lower_the_histogram_term_of_every_style_layer(tmp_path, weight_files):
    import optim
    cfg = make_cfg(style_layers=LAYERS, hist_loss_factor=1.0)
    args = preset_args(tmp_path, weight_files, dict(hist_loss_factor=1.0), S=64, N=10)
    content, style, init = synth.images(64)
    out = optim.optimize(content, [style], init.clone(), 10, args)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    ref = hr.build(content.double(), [style.double()], cfg, synth.vgg19_state_dict(dtype=torch.float64))
    before, after = ref.hist_terms(init.double()), ref.hist_terms(out.double())
    assert len(before) == 3
    for i in before:
        print(f"  style layer at {i}: h {before[i]:.6e} -> {after[i]:.6e}")
        assert after[i] < before[i], (i, before[i], after[i])
    assert rel_l2(out, init) > 1e-3  # (it moved)


def test_cli_with_the_preset_key(tmp_path, weight_files):
    """style.py --load_args hist.json --image_sizes 64 --num_iters 5 finishes, and its picture differs from the run's without the preset."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    preset = tmp_path / "hist.json"
    preset.write_text(json.dumps({"hist_loss_factor": 1.0}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    images = {}
    for label, extra in (("hist", ["--load_args", str(preset)]), ("plain", [])):
        out = tmp_path / label
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), *extra,
                            "--image_sizes", "64", "--num_iters", "5", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                            str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out)], cwd=PKG,
                           env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_64.png"]
        images[label] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["hist"].shape == (64, 64, 3)
    assert np.abs(images["hist"] - images["plain"]).max() > 0
