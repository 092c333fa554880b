"""style.img_vid end to end with the plan field clip_device at 0 (the reference's host loop) and at 1 (the clip stays on the device:
hip.gauss_wrap, hip.resize_bilinear, windows gathered on the device, frames out as 8-bit images), optim.optimize spied.

The job is the one of tests/test_cli_gpu.py::test_img_vid_frame_directories_end_to_end with `--num_frames 9` (the roll between scales is
real) and `--no_hist_match` (no global-RNG draw but the clip's noise), for `--init random` and `--init content`.  "theirs" is the host run:
scipy's fp32 filter and torch's fp32 interpolate.  Every bar is a distance from an fp64 restatement written here, relative to the host
code's own distance from it; both are measured and printed.  Values after the first optimisation get sanity bounds only: a few
optimisation steps amplify last-bit differences of their initial image (tests/test_cli_gpu.py's flow-cache test says why)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from conftest import rel_l2

pytestmark = pytest.mark.gpu

T, SIDE, SIZES = 9, 64, (32, 48)


def write_inputs(root):
    clip = root / "clip"
    clip.mkdir()
    g = torch.Generator().manual_seed(8)
    for t in range(4):
        Image.fromarray((torch.rand(40, 44, 3, generator=g) * 255).byte().numpy()).save(clip / f"s_{t:03d}.png")
    content = root / "content.png"
    Image.fromarray((torch.rand(SIDE, SIDE, 3, generator=g) * 255).byte().numpy()).save(content)
    scaling = root / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    return str(clip), str(content), str(scaling)


def run_img_vid(weight_files, inputs, out, init, device, monkeypatch):
    """One in-process job; returns the optimize calls as (initial clip on the CPU, result on the CPU, whether the initial clip was a device tensor)."""
    import config
    import optim
    import plan
    import style
    clip, content, scaling = inputs
    os.makedirs(out, exist_ok=True)
    args = config.get_args(["--transfer_type", "img_vid", "--content", content, "--style", clip, "--image_sizes", ",".join(str(s) for s in SIZES),
                            "--num_iters", "3,2", "--gram_frame_window", "3,3", "--num_frames", str(T), "--init", init, "--seed", "0",
                            "--style_layers", "relu1_1,relu2_1", "--content_layers", "relu2_2", "--model_file", weight_files["vgg19"],
                            "--disable_check", "--scaling_args", scaling, "--no_hist_match", "--output_dir", out])
    calls = []
    real_opt = optim.optimize

    def spy(content, styles, init, n, a, net=None, losses=None, **kw):
        init0 = init.detach().clone().cpu()
        res = real_opt(content, styles, init, n, a, net, losses, **kw)
        calls.append((init0, res.detach().clone().cpu(), bool(init.is_cuda), bool(res.is_cuda)))
        return res
    with monkeypatch.context() as m:
        m.setitem(plan.OVERRIDES, "clip_device", "1" if device else "0")
        m.setattr(optim, "optimize", spy)
        torch.manual_seed(0)
        style.img_vid(args)
    return calls, args


def tree(out):
    return {d: sorted(os.listdir(os.path.join(out, d))) for d in sorted(os.listdir(out))}


def first_init_f64(init, content_path):
    """The first optimize call's initial clip in fp64 from the seed's noise: noise * 255 in fp32 (both paths form it so), then float64."""
    import load
    import scipy.ndimage as ndi
    torch.manual_seed(0)
    x = (torch.randn((T, 3, SIDE, SIDE)) * 255).double()
    if init == "random":
        sig = [T, 0, SIDE / 32, SIDE / 32]
    else:
        x = load.preprocess(content_path).double().repeat([T, 1, 1, 1]) + x
        sig = [T, 0, 4, 4]
    clip = torch.from_numpy(ndi.gaussian_filter(x.numpy(), sig, mode="wrap"))
    return F.interpolate(clip, (SIZES[0], SIZES[0]), mode="bilinear", align_corners=False)


def between_scales(out1, blend, dtype):
    """Roll by 7 frames, temporal blend, resize to the second scale: in `dtype` with scipy and torch (float32 = the host chain's arithmetic)."""
    import scipy.ndimage as ndi
    p = out1.to(dtype)
    p = torch.cat((p[7:], p[:7]))
    p = torch.from_numpy(ndi.gaussian_filter(p.numpy(), [blend, 0, 0, 0], mode="wrap"))
    return F.interpolate(p, (SIZES[1], SIZES[1]), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("init", ("random", "content"))
def test_img_vid_with_the_clip_on_the_device(weight_files, tmp_path, monkeypatch, init):
    inputs = write_inputs(tmp_path)
    host_out, dev_out = str(tmp_path / "host"), str(tmp_path / "device")
    host_calls, _ = run_img_vid(weight_files, inputs, host_out, init, False, monkeypatch)
    calls, args = run_img_vid(weight_files, inputs, dev_out, init, True, monkeypatch)

    # structure
    assert len(calls) == len(host_calls) == 2
    frames = [f"frame_{t:05d}.png" for t in range(T)]
    assert tree(dev_out) == tree(host_out) == {"content_clip": frames, "content_clip_32": frames, "content_clip_48": frames}
    for (i_d, o_d, in_dev, out_dev), (i_h, o_h, in_host, out_host), side in zip(calls, host_calls, SIZES):
        assert i_d.shape == i_h.shape == o_d.shape == o_h.shape == (T, 3, side, side)
        assert all(bool(torch.isfinite(v).all()) for v in (i_d, o_d, i_h, o_h))
        assert in_dev and out_dev and not in_host and not out_host
    for d, side in (("content_clip_32", 32), ("content_clip_48", 48), ("content_clip", 48)):
        assert Image.open(os.path.join(dev_out, d, frames[0])).size == (side, side)

    # first call: the initial clip against fp64 from the same seed's noise
    ref0 = first_init_f64(init, inputs[1])
    d_dev, d_host = rel_l2(calls[0][0], ref0), rel_l2(host_calls[0][0], ref0)
    print(f"--init {init}: first initial clip vs fp64: device {d_dev:.3e}  host {d_host:.3e}  device vs host {rel_l2(calls[0][0], host_calls[0][0]):.3e}")
    assert d_dev <= 2 * d_host, (d_dev, d_host)

    # second scale: roll, blend, resize of the device run's OWN first result, against the fp32 host chain on the same tensor
    blend = float(args.temporal_blend)
    assert blend > 0
    ref1 = between_scales(calls[0][1], blend, torch.float64)
    d_dev, d_chain = rel_l2(calls[1][0], ref1), rel_l2(between_scales(calls[0][1], blend, torch.float32), ref1)
    print(f"--init {init}: second initial clip vs fp64: device {d_dev:.3e}  fp32 host chain {d_chain:.3e}")
    assert d_dev <= 2 * d_chain, (d_dev, d_chain)

    # later values: sanity bounds only
    for k in range(2):
        e = rel_l2(calls[k][1], host_calls[k][1])
        print(f"--init {init}: result of call {k}: device vs host {e:.3e}")
        assert e <= 0.5
    final = np.stack([np.asarray(Image.open(os.path.join(dev_out, "content_clip", f)), dtype=np.int32) for f in frames])
    final_host = np.stack([np.asarray(Image.open(os.path.join(host_out, "content_clip", f)), dtype=np.int32) for f in frames])
    assert final.std() > 1 and np.abs(final[0] - final[3]).max() > 0 and np.abs(final - final_host).mean() <= 20.0

    # resume: everything is finished - nothing is optimised, nothing is written
    def snapshot():
        return {(d, f): os.stat(os.path.join(dev_out, d, f)).st_mtime_ns for d, fs in tree(dev_out).items() for f in fs}
    before = snapshot()
    again, _ = run_img_vid(weight_files, inputs, dev_out, init, True, monkeypatch)
    assert again == [] and snapshot() == before
