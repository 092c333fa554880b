"""The shifted-Gram style loss (--shift_factor) end to end on the GPU: optim + the loss modules over the shifted Gram kernels against the
fp64 restatement (tests/shift_restatement.py).

Bars (those of tests/test_guided_style_gpu.py): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4; trajectories
relL2(ours, f64) <= max(1e-3, 2 relL2(restatement in fp32, f64))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import shift_restatement as sr
import synth
from conftest import NIN_FLAGS, NIN_LAYERS, PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4


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
    ref = sr.build(content.double(), [s.double() for s in styles], cfg, sd)
    total_r, losses_r, grad_r = ref.feval(init.double())
    net, losses, opt = prepared(args, content, styles, init, size)
    slots, total, grad = opt.feval()
    torch.cuda.synchronize()
    assert opt.engine is None
    order = loss_order(ref.spec)
    assert len(order) == len(losses)
    got = slots.cpu().double()
    for k, i in enumerate(order):
        want = float(losses_r[i]) if i in losses_r else 0.0
        print(f"  {losses[k].name}: {float(got[k]):.9e} (fp64 {want:.9e})")
        assert abs(float(got[k]) - want) <= TOL_LOSS * abs(want), (losses[k].name, float(got[k]), want)
    e = rel_l2(grad.cpu(), grad_r)
    print(f"  pixel gradient rel-L2 {e:.3e}")
    assert abs(float(total) - float(total_r)) <= TOL_LOSS * abs(float(total_r))
    assert e <= TOL_GRAD
    return ref, net, opt


def test_vgg19_at_128(weight_files):
    """relu1_1 (128) has the deltas [4, 16], relu2_1 (64) and relu3_1 (32) have [4], the deeper layers none."""
    cfg = make_cfg(shift_factor=0.5)
    args = product_args(weight_files, ["--shift_factor", "0.5"], S=128)
    content, style, init = synth.images(128)
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 128)
    assert [m.shift_target_deltas for m in net.style_losses] == [[4, 16], [4], [4], [], []]
    assert [len(m.shift_targets_x) for m in net.style_losses] == [2, 1, 1, 0, 0]
    i0 = [k for k, l in enumerate(ref.spec) if l.kind == "style"][0]
    first = net.style_losses[0]
    assert rel_l2(first.shift_targets_x[1].cpu(), ref.shift_targets[i0][(16, 0)]) <= 1e-5
    assert rel_l2(first.shift_targets_y[0].cpu(), ref.shift_targets[i0][(4, 1)]) <= 1e-5


def test_vgg19_40x56_two_styles_one_offers_a_delta_the_content_lacks(weight_files, capsys):
    """The 150 x 130 style image produces delta 16 at relu1_1; the 48 x 48 one and the 40 x 56 content do not: it is dropped and named."""
    cfg = make_cfg(style_blend_weights=[0.25, 0.75], shift_factor=0.5)
    args = product_args(weight_files, ["--style_blend_weights", "0.3,0.9", "--shift_factor", "0.5"], S=56, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 150, 130, generator=gen) * 255 - 120
    init = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    capsys.readouterr()
    ref, net, opt = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, 56)
    first = net.style_losses[0]
    assert first.shift_target_deltas == [4] and len(first.shift_targets_x) == 1 and len(first.shift_targets_y) == 1
    i0 = [k for k, l in enumerate(ref.spec) if l.kind == "style"][0]
    assert ref.shift_deltas[i0] == [4] and ref.dropped[i0] == [16]
    opt.feval()  # (named once, not per evaluation)
    err = capsys.readouterr().err
    assert err.count(f"{first.name}: shift 16 ") == 1, err


def test_nin_99_with_covariance(weight_files):
    cfg = make_cfg(use_covariance=True, shift_factor=0.5, **NIN_LAYERS)
    args = product_args(weight_files, NIN_FLAGS + ["--use_covariance", "--shift_factor", "0.5"], model="nin", S=99)
    content, style, init = synth.images(99)
    check_evaluation(cfg, args, synth.nin_state_dict(dtype=torch.float64), content, [style], init, 99)


def test_no_grad_norm_at_64(weight_files):
    cfg = make_cfg(normalize_gradients=False, shift_factor=0.5)
    args = product_args(weight_files, ["--no_grad_norm", "--shift_factor", "0.5"], S=64)
    content, style, init = synth.images(64)
    check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 64)


def test_two_frames_at_module_level_are_evaluated_per_frame():
    import loss
    gen = torch.Generator().manual_seed(7)
    C, H, W, s, sf = 8, 40, 44, 3.0, 0.5
    style = torch.relu(torch.randn(1, C, H, W, generator=gen))
    x = torch.relu(torch.randn(2, C, H, W, generator=gen) + 0.2)
    m = loss.StyleLoss(s, shift_factor=sf)
    m.name = "style_two_frames"
    m.mode, m.blend_weight = "capture", 1.0
    m(style.cuda())
    assert m.shift_target_deltas == [4]
    m.mode = "loss"
    xg = x.cuda().requires_grad_(True)
    m(xg)
    m.loss.backward()

    def terms(f):  # f: (C, H, W) fp64 -> [G / nelement, G_(4,x), G_(4,y)]
        flat = f.reshape(C, -1)
        return [flat @ flat.t() / f.nelement(), sr.shifted_gram(f, 0, 4), sr.shifted_gram(f, 1, 4)]

    targets = terms(style[0].double())
    x64 = x.double().requires_grad_(True)
    want = 0
    for b in range(2):
        t = [((g - tg) ** 2).mean() for g, tg in zip(terms(x64[b]), targets)]
        want = want + (t[0] + sf * (t[1] + t[2])) * s / 2
    want.backward()
    assert abs(float(m.loss.detach()) - float(want.detach())) <= TOL_LOSS * abs(float(want.detach()))
    assert rel_l2(xg.grad.cpu(), x64.grad) <= TOL_GRAD


def test_ten_lbfgs_iterations_vs_fp64(weight_files):
    import optim
    cfg = make_cfg(shift_factor=0.5)
    args = product_args(weight_files, ["--shift_factor", "0.5"], S=64, N=10)
    content, style, init = synth.images(64)
    ref64 = sr.optimize(content.double(), [style.double()], init.double(), 10, cfg, synth.vgg19_state_dict(dtype=torch.float64), torch.float64)
    ref32 = sr.optimize(content, [style], init, 10, cfg, synth.vgg19_state_dict(), torch.float32)
    out = optim.optimize(content, [style], init.clone(), 10, args)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    floor, err = rel_l2(ref32, ref64), rel_l2(out, ref64)
    print(f"lbfgs: relL2(ours, f64) {err:.3e}, relL2(restatement in fp32, f64) {floor:.3e}")
    assert err <= max(1e-3, 2 * floor), (err, floor)
    assert rel_l2(out, init) > 1e-3  # (it moved)


def test_shifted_nets_leave_the_engine_and_get_it_back_at_zero(weight_files):
    import engine
    import optim
    content, style, init = synth.images(64)
    net, losses, opt = prepared(product_args(weight_files, ["--shift_factor", "0.5"], S=64), content, [style], init, 64)
    assert opt.engine is None and optim._shifted(net) and optim._engine_of(net) is None
    opt.step()
    assert opt.engine is None
    with pytest.raises(engine.UnsupportedNet, match="shifted StyleLoss runs on the module path"):
        engine.StyleEngine(net, losses)
    for m in net.style_losses:
        m.shift_factor = 0
    args0 = product_args(weight_files, S=64)
    back = optim.PixelOptimizer(net, losses, init, args0)
    assert back.engine is not None
    _, _, fresh = prepared(args0, content, [style], init, 64)
    assert fresh.engine is not None
    a, b = back.feval(), fresh.feval()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_cli_with_a_shift_factor(tmp_path, weight_files):
    """style.py --shift_factor 1 --image_sizes 64 --num_iters 5 finishes, and its picture differs from the --shift_factor 0 run's."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    images = {}
    for sf in ("1", "0"):
        out = tmp_path / f"sf{sf}"
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), "--shift_factor", sf,
                            "--image_sizes", "64", "--num_iters", "5", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                            str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out)], cwd=PKG,
                           env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_64.png"]
        images[sf] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["1"].shape == (64, 64, 3)
    assert np.abs(images["1"] - images["0"]).max() > 0
