"""The device-resident temporal path of vid_img (plan field temporal_device = 1): csrc/warp.hip through the C ABI (hip.py) against the
reference's own outputs (tests/golden/flow_warp_map.npz, vid_flow_S64.npz) and against fp64 restatements written here, and
style.vid_img end to end with the field at 0 and at 1.

"theirs" below is the fp32 CPU code the reference runs (scipy's float32 gaussian_filter, torch's fp32 interpolate / grid_sample);
every bar is stated against its distance from the fp64 restatement, both distances are measured here and printed."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from conftest import GOLDEN, REPO, rel_l2, write_video_fixture

pytestmark = pytest.mark.gpu

FP32_ULP = 1.2e-7  # one fp32 unit in the last place of the grid's O(1) values: the floor of the warp-grid bar


def grid_f64(flow, size):
    """load.flow_warp_map (reference load.py:191-214) restated in fp64: scipy's gaussian_filter on float64, torch double interpolation."""
    import scipy.ndimage
    f = flow.astype(np.float64).copy()
    h, w = f.shape[:2]
    f[:, :, 0] /= w
    f[:, :, 1] /= h
    f = scipy.ndimage.gaussian_filter(f, [5, 5, 0])
    gx, gy = np.meshgrid(np.linspace(-1, 1, w), np.linspace(-1, 1, h))
    grid = torch.from_numpy(np.stack([gx, gy], axis=2) + f).unsqueeze(0)
    return F.interpolate(grid.permute(0, 3, 1, 2), size=tuple(size), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def sample_f64(x, grid):
    return F.grid_sample(x.double(), grid.double(), mode="bilinear", padding_mode="border", align_corners=False)


@pytest.fixture(scope="module")
def warp_fixture():
    return np.load(os.path.join(GOLDEN, "flow_warp_map.npz"))


def check_grid(flow, size, theirs, tag):
    import hip
    ref = grid_f64(flow, size)
    ours = hip.flow_warp_grid(torch.from_numpy(flow).cuda(), size)
    assert ours.shape == ref.shape and ours.dtype == torch.float32
    e_ours, e_theirs = rel_l2(ours.cpu(), ref), rel_l2(theirs, ref)
    print(f"warp grid {tag}: ours {e_ours:.3e}  theirs {e_theirs:.3e}  ours vs theirs {rel_l2(ours.cpu(), theirs):.3e}")
    assert torch.isfinite(ours).all()
    assert e_ours <= max(2 * e_theirs, FP32_ULP), (tag, e_ours, e_theirs)
    return ours


@pytest.mark.parametrize("key, size", [("warp_40x56", (40, 56)), ("warp_64x80", (64, 80))])
def test_warp_grid_against_the_reference_output(warp_fixture, key, size):
    check_grid(warp_fixture["flow"], size, torch.from_numpy(warp_fixture[key]), key)


@pytest.mark.parametrize("hw, size", [
    ((2, 2), (5, 7)),          # smallest plane: every tap is a reflection, many times over
    ((7, 19), (64, 80)),       # both sides shorter than the radius
    ((21, 20), (21, 20)),      # at the radius
    ((45, 130), (30, 64)),     # downscale, crosses tile edges (32 x 32 tiles)
    ((64, 64), (64, 64)),      # identity resize
])
def test_warp_grid_on_seeded_fields(tmp_path, hw, size):
    import load
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    yy, xx = np.meshgrid(np.linspace(0, 3, hw[0]), np.linspace(0, 3, hw[1]), indexing="ij")
    flow = np.stack([2.5 * np.sin(yy) * np.cos(xx), -1.5 * np.cos(yy)], axis=2) + rng.normal(size=hw + (2,))
    flow = flow.astype(np.float32)
    path = str(tmp_path / "f.flo")
    load.write_flow(flow, path)
    theirs = load.flow_warp_map(path, size)
    ours = check_grid(flow, size, theirs, f"{hw}->{size}")
    again = load.flow_warp_grid_device(path, size)  # the host entry: read_flo, upload, kernel
    assert torch.equal(ours, again)


def test_grid_sample_against_the_reference_output(warp_fixture):
    import hip
    x, grid = torch.from_numpy(warp_fixture["image"]), torch.from_numpy(warp_fixture["warp_64x80"])
    size = torch.tensor([80.0, 64.0], dtype=torch.float64)
    pos = ((grid.double() + 1) * size - 1) / 2
    outside = float(((pos < 0) | (pos > size - 1)).any(-1).float().mean())
    ref = sample_f64(x, grid)
    ours = hip.grid_sample_border(x.cuda(), grid.cuda()).cpu()
    theirs = torch.from_numpy(warp_fixture["warped"])
    e_ours, e_theirs = rel_l2(ours, ref), rel_l2(theirs, ref)
    print(f"grid_sample fixture: ours {e_ours:.3e}  theirs {e_theirs:.3e}  samples at or past the border {outside:.3f}")
    assert outside > 0.02  # the fixture exercises the clamp
    assert e_ours <= 2 * e_theirs, (e_ours, e_theirs)


def seeded_grid(gen, n, hw_in, hw_out):
    """Sampling positions where the kernel can go wrong: exact pixel centres, values at exactly -1 and 1, a tenth far outside."""
    (h, w), (H, W) = hw_in, hw_out
    grid = torch.rand(n, H, W, 2, generator=gen) * 2.2 - 1.1
    kind = torch.rand(n, H, W, generator=gen)
    cx = ((2 * torch.randint(0, w, (n, H, W), generator=gen) + 1).float() / w - 1)
    cy = ((2 * torch.randint(0, h, (n, H, W), generator=gen) + 1).float() / h - 1)
    centres = torch.stack([cx, cy], -1)
    grid = torch.where((kind < 0.2)[..., None], centres, grid)
    ends = torch.where(torch.rand(n, H, W, 2, generator=gen) < 0.5, -torch.ones(()), torch.ones(()))
    grid = torch.where(((kind >= 0.2) & (kind < 0.3))[..., None], ends, grid)
    far = torch.rand(n, H, W, 2, generator=gen) * 6 - 3
    grid = torch.where((kind >= 0.9)[..., None], far, grid)
    return grid.contiguous()


SAMPLE_CASES = [  # n, c, image (h, w), output (H, W)
    (1, 1, (1, 1), (1, 1)),
    (1, 3, (2, 3), (2, 3)),
    (2, 3, (33, 65), (33, 65)),
    (1, 3, (64, 80), (40, 56)),
    (2, 1, (64, 80), (40, 56)),
]


@pytest.mark.parametrize("n, c, hw_in, hw_out", SAMPLE_CASES)
def test_grid_sample_on_seeded_cases(n, c, hw_in, hw_out):
    import hip
    gen = torch.Generator().manual_seed(7 + n + 10 * c + hw_in[0])
    x = torch.randn(n, c, *hw_in, generator=gen) * 60
    grid = seeded_grid(gen, n, hw_in, hw_out)
    ref = sample_f64(x, grid)
    theirs = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
    ours = hip.grid_sample_border(x.cuda(), grid.cuda())
    assert ours.shape == ref.shape
    e_ours, e_theirs = rel_l2(ours.cpu(), ref), rel_l2(theirs, ref)
    print(f"grid_sample n={n} c={c} {hw_in}->{hw_out}: ours {e_ours:.3e}  theirs {e_theirs:.3e}")
    assert e_ours <= 2 * e_theirs, (e_ours, e_theirs)
    if hw_in == hw_out:  # the fused temporal blend: (1 - a) * blend + a * x in fp64, two fp32 roundings per element allowed
        a = 0.3
        blend = torch.randn(n, c, *hw_in, generator=gen) * 60
        warped, init = hip.grid_sample_border(x.cuda(), grid.cuda(), blend=blend.cuda(), blend_a=a)
        assert torch.equal(warped, ours)  # the second output changes no bit of the first
        want = (1 - a) * blend.double() + a * x.double()
        err = (init.cpu().double() - want).abs()
        print(f"  fused blend: largest relative error {float((err / want.abs().clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= FP32_ULP * want.abs()).all())


def test_mask_against_the_reference_masks(tmp_path):
    import hip
    import load
    g = np.load(os.path.join(GOLDEN, "vid_flow_S64.npz"))
    _, outdir = write_video_fixture(str(tmp_path))
    flow_dir = os.path.join(outdir, "clip_synth_style_256", "flow")
    # pass 2 runs the clip backwards: the pairs (0002, 0001), (0001, 0000), (0000, 0002)
    for prev, this in (("0002", "0001"), ("0001", "0000"), ("0000", "0002")):
        want = torch.from_numpy(g[f"tweights_2_{this}.png"])
        got = load.reliable_flow_weighting_device(os.path.join(flow_dir, f"backward_{prev}_{this}.png"), (64, 64))
        assert got.shape == want.shape
        d = float((got.cpu() - want).abs().max())
        print(f"mask backward_{prev}_{this}: largest difference {d:.3e}")
        assert d <= 1e-6
    # three channels and a real resize, against torch's fp32 interpolate of bytes / 255: both sides round a blend of values in
    # [0, 1] at most three times (6e-8 each), so they are within 4e-7 of each other
    m = torch.randint(0, 256, (37, 50, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    want = F.interpolate((m.permute(2, 0, 1).float() / 255.0).unsqueeze(0), size=(64, 41), mode="bilinear", align_corners=False)
    got = hip.mask_u8_resize(m.cuda(), (64, 41)).cpu()
    d = float((got - want).abs().max())
    print(f"mask 37x50x3 -> 64x41: largest difference {d:.3e}")
    assert got.shape == want.shape and d <= 4e-7


def test_reruns_are_bit_identical(warp_fixture):
    import hip
    flow = torch.from_numpy(warp_fixture["flow"]).cuda()
    x = torch.from_numpy(warp_fixture["image"]).cuda()
    blend = torch.flip(x, dims=(3,)).contiguous()
    mask = torch.randint(0, 256, (40, 56), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).cuda()
    first = None
    for _ in range(3):
        grid = hip.flow_warp_grid(flow, (64, 80))
        warped, init = hip.grid_sample_border(x, grid, blend=blend, blend_a=0.5)
        got = (grid, warped, init, hip.mask_u8_resize(mask, (64, 80)))
        if first is None:
            first = got
        assert all(torch.equal(a, b) for a, b in zip(first, got))


def test_wrappers_refuse_cpu_tensors_and_bad_shapes(warp_fixture):
    import hip
    flow, x = torch.from_numpy(warp_fixture["flow"]), torch.from_numpy(warp_fixture["image"])
    grid = torch.from_numpy(warp_fixture["warp_64x80"])
    with pytest.raises(hip.HipError):
        hip.flow_warp_grid(flow, (8, 8))
    with pytest.raises(hip.HipError):
        hip.grid_sample_border(x, grid)
    with pytest.raises(hip.HipError):
        hip.mask_u8_resize(torch.zeros(4, 4, dtype=torch.uint8), (4, 4))
    with pytest.raises(hip.HipError):  # the fused blend needs the output to have the image's size
        hip.grid_sample_border(x.cuda(), torch.zeros(1, 8, 8, 2).cuda(), blend=x.cuda(), blend_a=0.5)
    with pytest.raises(hip.HipError):
        hip.flow_warp_grid(flow.cuda(), (0, 8))


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def run_vid_img(weight_files, fdir, outdir, device, monkeypatch):
    """style.vid_img over the flow-cache fixture with the argument list of test_cli_gpu's flow-cache test; returns the optimize calls
    (file name, initial image, result) and the number of temporal-target calls."""
    import config
    import optim
    import plan
    import style
    scaling = os.path.join(os.path.dirname(weight_files["vgg19"]), "scaling-test.json")
    if not os.path.exists(scaling):
        with open(scaling, "w") as f:
            json.dump({"100000": {"gpu": "0", "multidevice": False}}, f)
    args = config.get_args(["--transfer_type", "vid_img", "--content", fdir, "--style", os.path.join(REPO, "tests", "synth_style_256.png"),
                            "--image_sizes", "64", "--num_iters", "8", "--passes_per_scale", "2", "--init", "prev_warp",
                            "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args", scaling, "--seed", "0",
                            "--no_hist_match", "--output_dir", outdir])
    calls, n_tt = [], [0]
    real_opt, real_tt = optim.optimize, optim.set_temporal_targets

    def spy(content, styles, init, n, a, net=None, losses=None, **kw):
        init0 = init.detach().clone().cpu()
        out = real_opt(content, styles, init, n, a, net, losses, **kw)
        calls.append((os.path.basename(a.output), init0, out.detach().clone().cpu()))
        return out

    def spy_tt(*a, **k):
        n_tt[0] += 1
        return real_tt(*a, **k)
    with monkeypatch.context() as m:
        m.setitem(plan.OVERRIDES, "temporal_device", "1" if device else "0")
        m.setattr(optim, "optimize", spy)
        m.setattr(optim, "set_temporal_targets", spy_tt)
        torch.manual_seed(0)
        style.vid_img(args)
    return calls, n_tt[0]


def test_vid_img_with_flow_cache_on_the_device(weight_files, tmp_path, monkeypatch):
    """The same job with the plan field at 0 and at 1: same call order, same files, same number of temporal targets; call 0's initial
    image (a prev_warp initialisation: one warp grid, one grid_sample) judged against an fp64 restatement of that warp from the same
    files; the later calls within the sanity bounds of test_cli_gpu's flow-cache test (whose comment says why tighter bounds mean
    nothing there).  Then the device job again into the same directory (skips everything), and once more after the last two PNGs
    of pass 2 were deleted (rewrites exactly those, with the bytes they had)."""
    import load
    g = np.load(os.path.join(GOLDEN, "vid_flow_S64.npz"))
    order = [str(x) for x in g["order"]]
    runs = {}
    for device in (False, True):
        root = tmp_path / ("device" if device else "host")
        root.mkdir()
        fdir, outdir = write_video_fixture(str(root))
        runs[device] = (fdir, outdir) + run_vid_img(weight_files, fdir, outdir, device, monkeypatch)
    fdir, outdir, calls, n_tt = runs[True]
    _, host_outdir, host_calls, host_n_tt = runs[False]
    frames_dir = os.path.join(outdir, "clip_synth_style_256", "64")
    assert [c[0] for c in calls] == order == [c[0] for c in host_calls]
    assert n_tt == host_n_tt == int(g["temporal_target_calls"])
    assert sorted(os.listdir(frames_dir)) == sorted(order) == sorted(os.listdir(os.path.join(host_outdir, "clip_synth_style_256", "64")))

    # call 0: frame 0000 warped along forward_0000_0001.flo
    flo = load.read_flo(os.path.join(outdir, "clip_synth_style_256", "flow", "forward_0000_0001.flo"))
    ref0 = sample_f64(load.preprocess(os.path.join(fdir, "0000.png")), grid_f64(flo, (64, 64)))
    d_dev, d_host = rel_l2(calls[0][1], ref0), rel_l2(host_calls[0][1], ref0)
    print(f"call 0 initial image vs fp64: device {d_dev:.3e}  host {d_host:.3e}")
    assert d_dev <= 2 * d_host, (d_dev, d_host)

    for k, (fname, init, out) in enumerate(calls):
        e_init, e_out = rel_l2(init, g["init_" + fname]), rel_l2(out, g["out_" + fname])
        png = np.asarray(Image.open(os.path.join(frames_dir, fname))).astype(np.int32)
        d = np.abs(png - g["png_" + fname].astype(np.int32))
        print(fname, "init", e_init, "out", e_out, "png max", d.max(), "mean", d.mean(),
              "| host run: init", rel_l2(host_calls[k][1], g["init_" + fname]), "out", rel_l2(host_calls[k][2], g["out_" + fname]))
        assert np.isfinite(out.numpy()).all() and np.isfinite(init.numpy()).all()
        assert e_init <= 0.3 and e_out <= 0.5 and d.mean() <= 20.0

    def snapshot():
        return {f: (open(os.path.join(frames_dir, f), "rb").read(), os.stat(os.path.join(frames_dir, f)).st_mtime_ns) for f in order}

    before = snapshot()
    again, _ = run_vid_img(weight_files, fdir, outdir, True, monkeypatch)
    assert again == [] and snapshot() == before  # every frame skipped, no file changed
    for f in order[-2:]:
        os.remove(os.path.join(frames_dir, f))
    resumed, _ = run_vid_img(weight_files, fdir, outdir, True, monkeypatch)
    assert [c[0] for c in resumed] == order[-2:]
    after = snapshot()
    assert sorted(os.listdir(frames_dir)) == sorted(order)
    for f in order:
        assert after[f][0] == before[f][0], f  # the bytes they had
        assert (after[f][1] == before[f][1]) == (f not in order[-2:]), f  # only the two were written
