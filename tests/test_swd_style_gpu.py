"""The sliced Wasserstein style loss (preset keys swd_factor / swd_directions / swd_seed / swd_bins / swd_knots) end to end on the GPU: optim +
the loss modules over the kernels of csrc/swd.hip against the restatement (tests/swd_restatement.py).  Synthetic VGG-19 weights and images at
64 x 64, three style layers (64 x 64, 32 x 32 and 16 x 16 pixels).

Bars (those of tests/test_feat_hist_style_gpu.py for the same comparison): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4.

The evaluation is compared with the restatement's under the SAME bin decisions, as in tests/test_feat_hist_style_gpu.py and for its reason:
the bin of a projected value is a decision and the matched value is not continuous across it.  hip.swd_project is wrapped for the
evaluation and a copy of every P it returns is kept; the restatement's own `decide` decides the bins on those fp32 values and the fp64
evaluation takes them as given (`swd_pinned`).  With hist_loss_factor > 0 the bins of the activations are pinned the same way.  The test
prints how many elements the pin moved."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import feat_hist_restatement as hr
import swd_restatement as wr
import synth
from conftest import PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4
LAYERS = "relu1_1,relu2_1,relu3_1"
REASON = "sliced-Wasserstein StyleLoss runs on the module path"

# configuration -> (restatement fields, preset keys, flags)
CONFIGS = {
    "defaults": (dict(swd_factor=1.0), dict(swd_factor=1.0), []),
    "directions16-bins16": (dict(swd_factor=1.0, swd_directions=16, swd_bins=16), dict(swd_factor=1.0, swd_directions=16, swd_bins=16), []),
    "factor0.5-seed3": (dict(swd_factor=0.5, swd_seed=3), dict(swd_factor=0.5, swd_seed=3), []),
    "with-histogram-mirrors-shift-covariance": (dict(swd_factor=1.0, hist_loss_factor=1.0, flip_factor=0.5, shift_factor=0.5, use_covariance=True),
                                                dict(swd_factor=1.0, hist_loss_factor=1.0, flip_factor=0.5),
                                                ["--shift_factor", "0.5", "--use_covariance"]),
}


def preset_args(tmp_path, weight_files, preset, extra=(), **kw):
    """The namespace a user gets from --load_args with the preset keys (there is no flag for them)."""
    path = tmp_path / "swd.json"
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
    import hip
    from oracle.style_oracle import loss_order
    ref = wr.build(content.double(), [s.double() for s in styles], cfg, sd)
    net, losses, opt = prepared(args, content, styles, init, size)
    acts, projections = [], []  # what the style modules get, and every P of the evaluation, in network order
    hooks = [m.register_forward_pre_hook(lambda mod, inp: acts.append(inp[0].detach().cpu())) for m in net.style_losses]
    real = hip.swd_project

    def recording(*a, **k):
        out = real(*a, **k)
        projections.append(out[0].clone())
        return out

    hip.swd_project = recording
    try:
        slots, total, grad = opt.feval()
        torch.cuda.synchronize()
    finally:
        hip.swd_project = real
        for h in hooks:
            h.remove()
    assert opt.engine is None
    style_slots = ref.style_slots()
    assert len(projections) == len(acts) == len(style_slots) and all(a.shape[0] == 1 for a in acts)
    swd_pinned = {i: hr.decide(p.cpu(), ref.swd_bins)[2] for i, p in zip(style_slots, projections)}
    pinned = {i: hr.decide(a[0], ref.bins)[2] for i, a in zip(style_slots, acts)} if ref.hist_loss_factor > 0 else None
    total_r, losses_r, grad_r = ref.feval(init.double(), pinned=pinned, swd_pinned=swd_pinned)
    own = ref.net._forward(init.double())[0]
    moved = {i: int((hr.decide(wr.project(own[i][0], ref.swd_dirs[i]), ref.swd_bins)[2] != swd_pinned[i]).sum()) for i in style_slots}
    print(f"  projected elements whose bin the fp32 run and the fp64 network decide differently, per style layer: {moved}")
    for index, (i, m) in enumerate(zip(style_slots, net.style_losses)):
        assert m.swd_index == index and torch.equal(m._swd_dirs[0].cpu(), ref.swd_dirs[i])
        assert torch.equal(m._swd_dirs[1].cpu(), ref.swd_dirs[i].t())
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
    slots = ref.style_slots()
    assert len(slots) == len(net.style_losses) == 3
    for i, m in zip(slots, net.style_losses):
        D = ref.swd_directions or m.target.shape[0]
        assert tuple(m.swd_target.shape) == tuple(ref.swd_targets[i].shape) == (D, ref.swd_knots)
        assert rel_l2(m.swd_target.cpu(), ref.swd_targets[i]) <= 1e-5, m.name
        assert bool((m.swd_target[:, 1:] >= m.swd_target[:, :-1]).all())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vgg19_at_64(tmp_path, weight_files, name):
    over, preset, flags = CONFIGS[name]
    cfg = make_cfg(style_layers=LAYERS, **over)
    args = preset_args(tmp_path, weight_files, preset, flags, S=64)
    content, style, init = synth.images(64)
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 64)
    check_targets(ref, net)


def test_two_styles_of_different_sizes_with_blend_weights(tmp_path, weight_files):
    cfg = make_cfg(style_layers=LAYERS, style_blend_weights=[0.25, 0.75], swd_factor=1.0)
    args = preset_args(tmp_path, weight_files, dict(swd_factor=1.0), ["--style_blend_weights", "0.3,0.9"], S=64, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content, _, init = synth.images(64)
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 90, 70, generator=gen) * 255 - 120
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, 64)
    check_targets(ref, net)


def test_factor_zero_gives_the_bits_of_a_run_without_the_key(tmp_path, weight_files):
    content, style, init = synth.images(64)
    _, _, with_key = prepared(preset_args(tmp_path, weight_files, dict(swd_factor=0, swd_bins=64, swd_directions=8), S=64), content, [style], init, 64)
    _, _, without = prepared(product_args(weight_files, ["--style_layers", LAYERS], S=64), content, [style], init, 64)
    assert with_key.engine is not None and without.engine is not None  # both on the fused engine
    assert all(m.swd_target is None and m._swd_dirs is None for m in with_key.net.style_losses)
    a, b = with_key.feval(), without.feval()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_two_frames_at_module_level_are_evaluated_per_frame():
    import loss
    gen = torch.Generator().manual_seed(7)
    C, D, H, W, s, sf, bins, knots = 8, 5, 13, 18, 3.0, 0.5, 64, 32
    style = torch.relu(2 * torch.randn(2, C, H + 2, W + 1, generator=gen) + 1)
    x = torch.relu(torch.randn(2, C, H, W, generator=gen) + 0.3)
    m = loss.StyleLoss(s)
    m.name = "style_two_frames"
    m.swd_factor, m.swd_directions, m.swd_bins, m.swd_knots, m.swd_seed, m.swd_index = sf, D, bins, knots, 2, 1
    m.mode, m.blend_weight = "capture", 1.0
    m(style.cuda())
    assert tuple(m.swd_target.shape) == (D, knots)
    m.mode = "loss"
    xg = x.cuda().requires_grad_(True)
    projections = []
    import hip
    real = hip.swd_project

    def recording(*a, **k):
        out = real(*a, **k)
        projections.append(out[0].clone())
        return out

    hip.swd_project = recording
    try:
        m(xg)
    finally:
        hip.swd_project = real
    m.loss.backward()
    assert len(projections) == 2

    def gram(f):
        flat = f.reshape(C, -1)
        return flat @ flat.t() / f.nelement()

    v = wr.directions(C, D, 2, 1)
    assert torch.equal(m._swd_dirs[0].cpu(), v)
    s64 = style.double()
    g_target = (gram(s64[0]) + gram(s64[1])) / 2   # blend weight x G / frames, per frame
    w_target = (wr.table(s64[0], v, knots) + wr.table(s64[1], v, knots)) / 2
    assert rel_l2(m.swd_target.cpu(), w_target) <= 1e-6
    x64 = x.double().requires_grad_(True)
    want = 0
    for b in range(2):
        pin = hr.decide(projections[b].cpu(), bins)[2]
        want = want + (((gram(x64[b]) - g_target) ** 2).mean() + sf * wr.term(x64[b], v, w_target, bins, pin)) * s / 2
    want.backward()
    assert abs(float(m.loss.detach()) - float(want.detach())) <= TOL_LOSS * abs(float(want.detach()))
    assert rel_l2(xg.grad.cpu(), x64.grad) <= TOL_GRAD


@pytest.mark.parametrize("terms_engine", [0, 1])
def test_the_route_is_the_module_path_with_its_reason(tmp_path, weight_files, terms_engine):
    import engine
    import optim
    content, style, init = synth.images(64)
    preset = dict(swd_factor=1.0, terms_engine=terms_engine)
    net, losses, opt = prepared(preset_args(tmp_path, weight_files, preset, S=64), content, [style], init, 64)
    assert all(bool(m.terms_engine) == bool(terms_engine) for m in net.style_losses)
    assert opt.engine is None and optim._sliced(net) and optim._engine_of(net) is None
    assert optim._terms_on_module_path(net) == REASON and optim._terms_on_module_path(losses) == REASON
    opt.step()
    assert opt.engine is None
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        engine.StyleEngine(net, losses)
    for m in net.style_losses:  # back at 0 the same network takes the engine again
        m.swd_factor = 0
    assert optim._terms_on_module_path(net) is None and not optim._style_targets_missing(net)
    back = optim.PixelOptimizer(net, losses, init, product_args(weight_files, ["--style_layers", LAYERS], S=64))
    assert back.engine is not None
    back.feval()
    net.style_losses[0].swd_factor = 1.0  # switched on again behind the engine's back: it refuses the evaluation
    with pytest.raises(engine.UnsupportedNet, match=REASON):
        back.engine.feval(back.x, capture=False)


def test_cli_three_lbfgs_iterations_with_the_preset_key(tmp_path, weight_files):
    """style.py --load_args swd.json --image_sizes 64 --num_iters 3 finishes on the module path; the losses it prints are finite and fall."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    preset = tmp_path / "swd.json"
    preset.write_text(json.dumps({"swd_factor": 1.0}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), "--load_args", str(preset),
                        "--image_sizes", "64", "--num_iters", "3", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                        str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out), "--print_iter", "1",
                        "--verbose"], cwd=PKG, env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["content_style_64.png"]
    losses = [float(v) for v in re.findall(r"Iteration \d+ / \S+, Loss: (\S+)", r.stdout)]
    print(f"  losses: {losses}")
    assert len(losses) == 2 and all(np.isfinite(losses))  # (optim.lbfgs_moves: three iterations are two moves, as under the reference's driver)
    assert losses[-1] < losses[0]
