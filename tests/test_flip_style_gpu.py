"""The mirrored-Gram style loss (preset keys flip_factor / rotation_factor) end to end on the GPU: optim + the loss modules over the mirrored
Gram kernels against the fp64 restatement (tests/flip_restatement.py).

Bars (those of tests/test_shift_style_gpu.py): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4; trajectories
relL2(ours, f64) <= max(1e-3, 2 relL2(restatement in fp32, f64))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import flip_restatement as fr
import synth
from conftest import PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4

# configuration -> (restatement fields, preset keys, flags)
CONFIGS = {
    "flip": (dict(flip_factor=0.5), dict(flip_factor=0.5), []),
    "rotation": (dict(rotation_factor=0.5), dict(rotation_factor=0.5), []),
    "all-with-shift-covariance": (dict(flip_factor=0.5, rotation_factor=0.25, shift_factor=0.5, use_covariance=True),
                                  dict(flip_factor=0.5, rotation_factor=0.25), ["--shift_factor", "0.5", "--use_covariance"]),
}


def preset_args(tmp_path, weight_files, preset, extra=(), **kw):
    """The namespace a user gets from --load_args with the preset keys (there is no flag for them)."""
    path = tmp_path / "sym.json"
    path.write_text(json.dumps(preset))
    return product_args(weight_files, ["--load_args", str(path)] + list(extra), **kw)


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
    ref = fr.build(content.double(), [s.double() for s in styles], cfg, sd)
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


def check_targets(ref, net, kinds):
    slots = [k for k, l in enumerate(ref.spec) if l.kind == "style"]
    assert len(slots) == len(net.style_losses) == 5
    for i, m in zip(slots, net.style_losses):  # every style layer has the terms, down to relu5_1's few pixels
        assert sorted(m.flip_targets) == sorted(kinds) == sorted(ref.flip_targets[i])
        for k in kinds:
            assert torch.equal(m.flip_targets[k], m.flip_targets[k].t())
            assert rel_l2(m.flip_targets[k].cpu(), ref.flip_targets[i][k]) <= 1e-5, (m.name, k)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vgg19_at_64(tmp_path, weight_files, name):
    over, preset, flags = CONFIGS[name]
    cfg = make_cfg(**over)
    args = preset_args(tmp_path, weight_files, preset, flags, S=64)
    content, style, init = synth.images(64)
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, 64)
    check_targets(ref, net, ref.kinds)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vgg19_40x56_two_styles_of_different_sizes(tmp_path, weight_files, name):
    """A mirror exists for every map: no list to reconcile between the 48 x 48 and the 150 x 130 style image and the 40 x 56 working image
    (odd layer sizes further down: 5 x 7 at relu4_1, 2 x 3 at relu5_1)."""
    over, preset, flags = CONFIGS[name]
    cfg = make_cfg(style_blend_weights=[0.25, 0.75], **over)
    args = preset_args(tmp_path, weight_files, preset, ["--style_blend_weights", "0.3,0.9"] + flags, S=56, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 150, 130, generator=gen) * 255 - 120
    init = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, 56)
    check_targets(ref, net, ref.kinds)


def test_two_frames_at_module_level_are_evaluated_per_frame():
    import loss
    gen = torch.Generator().manual_seed(7)
    C, H, W, s, ff, rf = 8, 13, 18, 3.0, 0.5, 0.25
    style = torch.relu(torch.randn(2, C, H, W, generator=gen))
    x = torch.relu(torch.randn(2, C, H, W, generator=gen) + 0.2)
    m = loss.StyleLoss(s, flip_factor=ff, rotation_factor=rf)
    m.name = "style_two_frames"
    m.mode, m.blend_weight = "capture", 1.0
    m(style.cuda())
    assert sorted(m.flip_targets) == [0, 1, 2]
    m.mode = "loss"
    xg = x.cuda().requires_grad_(True)
    m(xg)
    m.loss.backward()

    def terms(f):  # f: (C, H, W) fp64 -> [G / nelement, G_LR, G_UD, G_180]
        flat = f.reshape(C, -1)
        return [flat @ flat.t() / f.nelement()] + [fr.mirrored_gram(f, k) for k in (fr.LR, fr.UD, fr.ROT180)]

    targets = [sum(t) / 2 for t in zip(terms(style[0].double()), terms(style[1].double()))]  # blend weight x G / frames, per frame
    x64 = x.double().requires_grad_(True)
    want = 0
    for b in range(2):
        t = [((g - tg) ** 2).mean() for g, tg in zip(terms(x64[b]), targets)]
        want = want + (t[0] + ff * (t[1] + t[2]) + rf * t[3]) * s / 2
    want.backward()
    assert abs(float(m.loss.detach()) - float(want.detach())) <= TOL_LOSS * abs(float(want.detach()))
    assert rel_l2(xg.grad.cpu(), x64.grad) <= TOL_GRAD


def test_ten_lbfgs_iterations_vs_fp64(tmp_path, weight_files):
    import optim
    over = dict(flip_factor=0.5, rotation_factor=0.25)
    cfg = make_cfg(**over)
    args = preset_args(tmp_path, weight_files, over, S=64, N=10)
    content, style, init = synth.images(64)
    ref64 = fr.optimize(content.double(), [style.double()], init.double(), 10, cfg, synth.vgg19_state_dict(dtype=torch.float64), torch.float64)
    ref32 = fr.optimize(content, [style], init, 10, cfg, synth.vgg19_state_dict(), torch.float32)
    out = optim.optimize(content, [style], init.clone(), 10, args)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    floor, err = rel_l2(ref32, ref64), rel_l2(out, ref64)
    print(f"lbfgs: relL2(ours, f64) {err:.3e}, relL2(restatement in fp32, f64) {floor:.3e}")
    assert err <= max(1e-3, 2 * floor), (err, floor)
    assert rel_l2(out, init) > 1e-3  # (it moved)


@pytest.mark.parametrize("preset", [dict(flip_factor=0.5), dict(rotation_factor=0.5)], ids=["flip", "rotation"])
def test_mirrored_nets_leave_the_engine_and_get_it_back_at_zero(tmp_path, weight_files, preset):
    import engine
    import optim
    content, style, init = synth.images(64)
    net, losses, opt = prepared(preset_args(tmp_path, weight_files, preset, S=64), content, [style], init, 64)
    assert opt.engine is None and optim._mirrored(net) and not optim._shifted(net) and optim._engine_of(net) is None
    opt.step()
    assert opt.engine is None
    with pytest.raises(engine.UnsupportedNet, match="mirrored StyleLoss runs on the module path"):
        engine.StyleEngine(net, losses)
    for m in net.style_losses:
        m.flip_factor = m.rotation_factor = 0
    args0 = product_args(weight_files, S=64)
    assert not optim._mirrored(net) and not optim._style_targets_missing(net)
    back = optim.PixelOptimizer(net, losses, init, args0)
    assert back.engine is not None
    _, _, fresh = prepared(args0, content, [style], init, 64)
    assert fresh.engine is not None
    a, b = back.feval(), fresh.feval()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # both factors switched on after that capture: one mirror's target is missing, and the engine built meanwhile refuses the evaluation
    net.style_losses[0].flip_factor = net.style_losses[0].rotation_factor = 0.5
    assert optim._style_targets_missing(net) and optim._engine_of(net) is None
    with pytest.raises(engine.UnsupportedNet, match="mirrored StyleLoss runs on the module path"):
        back.engine.feval(back.x, capture=False)


def test_cli_with_the_preset_keys(tmp_path, weight_files):
    """style.py --load_args sym.json --image_sizes 64 --num_iters 5 finishes, and its picture differs from the run's without the preset."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    preset = tmp_path / "sym.json"
    preset.write_text(json.dumps({"flip_factor": 1.0, "rotation_factor": 0.5}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    images = {}
    for label, extra in (("sym", ["--load_args", str(preset)]), ("plain", [])):
        out = tmp_path / label
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), *extra,
                            "--image_sizes", "64", "--num_iters", "5", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                            str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out)], cwd=PKG,
                           env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_64.png"]
        images[label] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["sym"].shape == (64, 64, 3)
    assert np.abs(images["sym"] - images["plain"]).max() > 0
