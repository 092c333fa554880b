"""The guided style loss end to end on the GPU: optim + the loss modules over the guided Gram kernels against the fp64 restatement
(tests/guided_restatement.py).

Bars (the survey's for the HIP path): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4; trajectories
relL2(ours, f64) <= max(1e-3, 2 relL2(restatement in fp32, f64))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import guided_restatement as gr
import synth
from conftest import NIN_FLAGS, NIN_LAYERS, PKG, make_cfg, product_args, rel_l2

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-4


def halves(R, H, W, vertical=True):
    """R hard bands (one-hot guides) over an H x W image."""
    g = torch.zeros(R, H, W)
    n = W if vertical else H
    for r in range(R):
        lo, hi = r * n // R, (r + 1) * n // R
        if vertical:
            g[r, :, lo:hi] = 1
        else:
            g[r, lo:hi, :] = 1
    return g


def prepared(args, content, styles, init, guides, size):
    """The network as optim.optimize prepares it, and the optimiser that evaluates it."""
    import models
    import optim
    optim.set_model_args(args, size)
    net, losses = models.load_model(args)
    optim.set_content_targets(net, content, args)
    optim.set_style_targets(net, styles, args, style_guides=None if guides is None else guides[1])
    if guides is not None:
        for m in net.style_losses:
            m.guide = guides[0].cuda()
    for m in losses:
        m.mode = "loss"
    return net, losses, optim.PixelOptimizer(net, losses, init, args)


def check_evaluation(cfg, args, sd, content, styles, init, guides, size):
    from oracle.style_oracle import loss_order
    ref = gr.build(content.double(), [s.double() for s in styles], cfg, sd, guides)
    total_r, losses_r, grad_r = ref.feval(init.double(), None if guides is None else guides[0])
    net, losses, opt = prepared(args, content, styles, init, guides, size)
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


def test_vgg19_two_regions_at_64(weight_files):
    cfg = make_cfg()
    args = product_args(weight_files, S=64)
    content, style, init = synth.images(64)
    guides = (halves(2, 64, 64), [halves(2, 64, 64, vertical=False)])
    check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [style], init, guides, 64)


def test_vgg19_40x56_two_styles_three_regions_one_absent(weight_files):
    """Region 2 is absent from the second style image: its target comes from the first one alone (weight 0.25 / 0.25)."""
    cfg = make_cfg(style_blend_weights=[0.25, 0.75])
    args = product_args(weight_files, ["--style_blend_weights", "0.3,0.9"], S=56, styles=("s1.png", "s2.png"))
    gen = torch.Generator().manual_seed(11)
    content = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 36, 60, generator=gen) * 255 - 120
    init = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    g2 = torch.zeros(3, 36, 60)
    g2[0, :, :24], g2[1, :, 24:] = 1, 1
    guides = (halves(3, 40, 56), [halves(3, 48, 48, vertical=False), g2])
    ref, net, _ = check_evaluation(cfg, args, synth.vgg19_state_dict(dtype=torch.float64), content, [s1, s2], init, guides, 56)
    first = net.style_losses[0]
    assert first.guided_weight == pytest.approx([1.0, 1.0, 0.25])
    i0 = [k for k, l in enumerate(ref.spec) if l.kind == "style"][0]
    assert rel_l2(first.guided_targets()[0].cpu(), ref.style_targets[i0]) <= 1e-5


def test_nin_99_with_covariance(weight_files):
    cfg = make_cfg(use_covariance=True, **NIN_LAYERS)
    args = product_args(weight_files, NIN_FLAGS + ["--use_covariance"], model="nin", S=99)
    content, style, init = synth.images(99)
    soft = torch.rand(2, 99, 99, generator=torch.Generator().manual_seed(3))
    guides = (halves(2, 99, 99), [soft])
    check_evaluation(cfg, args, synth.nin_state_dict(dtype=torch.float64), content, [style], init, guides, 99)


@pytest.mark.parametrize("variant", ["default", "covariance"])
def test_all_ones_guides_match_the_unguided_module_path(weight_files, variant):
    cov = variant == "covariance"
    cfg = make_cfg(use_covariance=cov)
    flags = ["--use_covariance"] if cov else []
    content, style, init = synth.images(64)
    ones = (torch.ones(1, 64, 64), [torch.ones(1, 64, 64)])
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    check_evaluation(cfg, product_args(weight_files, flags, S=64), sd, content, [style], init, ones, 64)
    net, losses, opt = prepared(product_args(weight_files, flags, S=64), content, [style], init, None, 64)
    slots_u, total_u, grad_u = opt._feval_modules()
    net, losses, opt = prepared(product_args(weight_files, flags, S=64), content, [style], init, ones, 64)
    slots_g, total_g, grad_g = opt.feval()
    torch.cuda.synchronize()
    for a, b in zip(slots_g.cpu().tolist(), slots_u.cpu().tolist()):
        assert abs(a - b) <= TOL_LOSS * abs(b)
    assert rel_l2(grad_g.cpu(), grad_u.cpu()) <= TOL_GRAD


def test_guided_nets_leave_the_engine_and_plain_nets_keep_it(weight_files):
    content, style, init = synth.images(64)
    guides = (halves(2, 64, 64), [halves(2, 64, 64)])
    for opt_name in ("lbfgs", "adam"):
        args = product_args(weight_files, optimizer=opt_name, S=64)
        net, losses, opt = prepared(args, content, [style], init, guides, 64)
        opt.step()
        assert opt.engine is None
        net, losses, opt = prepared(product_args(weight_files, optimizer=opt_name, S=64), content, [style], init, None, 64)
        opt.step()
        assert opt.engine is not None
    import engine
    net, losses, _ = prepared(product_args(weight_files, S=64), content, [style], init, guides, 64)
    with pytest.raises(engine.UnsupportedNet, match="guided StyleLoss runs on the module path"):
        engine.StyleEngine(net, losses)


@pytest.mark.parametrize("opt_name", ["lbfgs", "adam"])
def test_five_iterations_vs_fp64(weight_files, opt_name):
    import optim
    cfg = make_cfg(optimizer=opt_name)
    args = product_args(weight_files, optimizer=opt_name, S=64, N=5)
    content, style, init = synth.images(64)
    guides = (halves(2, 64, 64), [halves(2, 64, 64, vertical=False)])
    ref64 = gr.optimize(content.double(), [style.double()], init.double(), 5, cfg, synth.vgg19_state_dict(dtype=torch.float64), guides, torch.float64)
    ref32 = gr.optimize(content, [style], init, 5, cfg, synth.vgg19_state_dict(), guides, torch.float32)
    out = optim.optimize(content, [style], init.clone(), 5, args, guides=guides)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    floor, err = rel_l2(ref32, ref64), rel_l2(out, ref64)
    print(f"{opt_name}: relL2(ours, f64) {err:.3e}, relL2(restatement in fp32, f64) {floor:.3e}")
    assert err <= max(1e-3, 2 * floor), (err, floor)
    assert rel_l2(out, init) > 1e-3  # (it moved)


def test_optimize_refuses_guides_on_frame_batches(weight_files):
    import optim
    args = product_args(weight_files, S=32)
    x = synth.frames(2, 32)
    guides = (torch.ones(1, 32, 32), [torch.ones(1, 32, 32)])
    with pytest.raises(NotImplementedError, match="guides"):
        optim.optimize(x[:1], [x[:1]], x, 1, args, guides=guides)


def test_cli_with_mask_preset(tmp_path, weight_files):
    """style.py with a --load_args preset that names masks: two scales that end at 64 pixels (48, then 64: a scale whose PNG exists is
    taken as finished, so the two sizes differ), PNGs written, and the result differs from the unguided run in both regions."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    rng = np.random.RandomState(4)
    content = tmp_path / "content.png"
    style = tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    cmask = np.zeros((64, 64, 3), np.uint8)
    cmask[:, 32:] = (255, 255, 255)
    smask = np.zeros((40, 40, 3), np.uint8)  # (a mask need not have its image's size)
    smask[20:] = (255, 255, 255)
    Image.fromarray(cmask).save(tmp_path / "cmask.png")
    Image.fromarray(smask).save(tmp_path / "smask.png")
    common = dict(image_sizes="48,64", num_iters="6,4", model_file=weight_files["vgg19"], disable_check=True, scaling_args=str(scaling), seed=0,
                  no_hist_match=True, init="content")
    (tmp_path / "guided.json").write_text(json.dumps(dict(common, content_mask=str(tmp_path / "cmask.png"), style_masks=[str(tmp_path / "smask.png")])))
    (tmp_path / "plain.json").write_text(json.dumps(common))
    images = {}
    for name in ("guided", "plain"):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), "--load_args",
                            str(tmp_path / f"{name}.json"), "--output_dir", str(out)], cwd=PKG, env=dict(os.environ, PYTHONPATH=PKG),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_48.png", "content_style_64.png"]
        images[name] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["guided"].shape == (64, 64, 3)
    diff = np.abs(images["guided"] - images["plain"])
    assert diff[:, :32].max() > 0 and diff[:, 32:].max() > 0
