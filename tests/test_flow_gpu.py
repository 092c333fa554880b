"""Optical flow for vid_img (--flow_models tvl1) on the MI355X: every csrc/flow.hip kernel against the fp64 restatement of its step
(tests/flow_restatement.py), the temporally blocked TV-L1 kernel bit for bit against single-step launches, whole estimates against
the fp64 oracle, the reliability mask pixel for pixel against the reference's (tests/golden/flow_consistency.npz), rerun / graph
replay determinism, the largest frame, and style.py's vid_img end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_restatement as R
from conftest import GOLDEN, PKG, REPO, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture
def stream():
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        yield s
    s.synchronize()


def _rand(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _state(h, w, seed):
    s = torch.cat([_rand((2, h, w), -2, 2, seed), _rand((4, h, w), -0.9, 0.9, seed + 1)])
    f = torch.cat([_rand((2, h, w), -30, 30, seed + 2), _rand((1, h, w), -40, 40, seed + 3)])
    # a few pixels with a vanishing gradient (the |grad|^2 < 1e-10 branch)
    f[:2, ::7, ::5] = 0
    return s, f


def test_grey_and_pyramid_against_fp64(stream):
    import hip
    rng = np.random.default_rng(0)
    for h, w in ((37, 53), (2, 3), (64, 1), (129, 96)):
        rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        g = hip.flow_grey(torch.from_numpy(rgb).cuda())
        assert rel_l2(g.cpu(), R.grey(rgb)) <= 2e-7
        img = _rand((h, w), 0, 255, h * w)
        d = hip.flow_pyr_down(img.cuda())
        assert tuple(d.shape) == ((h + 1) // 2, (w + 1) // 2)
        assert rel_l2(d.cpu(), R.pyr_down(img.double())) <= 1e-6


def test_warp_prep_against_fp64(stream):
    import hip
    for h, w in ((37, 53), (1, 40), (40, 1), (96, 128)):
        i0, i1 = _rand((h, w), 0, 255, 1), _rand((h, w), 0, 255, 2)
        u = _rand((2, h, w), -4, 4, 3)
        got = hip.flow_warp_prep(i0.cuda(), i1.cuda(), u.cuda()).cpu()
        want = R.warp_prep(i0.double(), i1.double(), u.double())
        for c in range(3):
            # the sample position x + u is rounded to fp32 first (1 ulp of 128 = 7.6e-6 px, times gradients of ~30 per px):
            # measured up to 3.7e-6 at 96 x 128
            assert rel_l2(got[c], want[c]) <= 1e-5, (h, w, c, rel_l2(got[c], want[c]))


def test_median_and_upsample_against_fp64(stream):
    import hip
    for h, w in ((37, 53), (1, 1), (3, 70), (64, 64)):
        x = _rand((2, h, w), -5, 5, 7)
        x[:, ::3] = torch.round(x[:, ::3])  # ties
        assert torch.equal(hip.flow_median5(x.cuda()).cpu(), R.median5(x))  # an exact selection
        for H, W in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1)):
            if H < 1 or W < 1:
                continue
            up = hip.flow_upsample(x.cuda(), H, W, 2.0).cpu()
            # (the source coordinate is computed in fp32, as ATen's own fp32 kernel does: measured up to 3.9e-6)
            assert rel_l2(up, R.upsample(x.double(), H, W, 2.0)) <= 1e-5


def test_tvl1_step_against_fp64(stream):
    import hip
    for h, w in ((37, 53), (1, 17), (17, 1), (2, 2), (128, 96)):
        s, f = _state(h, w, 11)
        got = hip.flow_tvl1_step(f.cuda(), s.cuda()).cpu()
        want = R.tv_step(f.double(), s.double())
        for c in range(6):
            assert rel_l2(got[c], want[c]) <= 1e-6, (h, w, c, rel_l2(got[c], want[c]))


@pytest.mark.parametrize("hw", [(1, 300), (300, 1), (2, 2), (31, 61), (97, 131), (1080, 1920)])
def test_blocked_iterations_are_bit_identical_to_single_steps(stream, hw):
    """k iterations in one launch of the temporally blocked kernel = k launches of the single-step kernel, bit for bit, for every
    tile-edge geometry (frames narrower than a tile, sides that are not multiples of 32, halos that leave the frame)."""
    import hip
    h, w = hw
    s, f = _state(h, w, 5)
    s, f = s.cuda(), f.cuda()
    for k in (1, 2, 5, 8, 16):
        ref = s
        for _ in range(k):
            ref = hip.flow_tvl1_step(f, ref)
        got = hip.flow_tvl1_step(f, s, k=k)
        assert torch.equal(got, ref), (hw, k, int((got != ref).sum()))
    # and a run of blocked launches chained like maua_flow_tvl1 does (k = 8, remainder 4)
    a, b = s, s
    for _ in range(20):
        a = hip.flow_tvl1_step(f, a)
    for k in (8, 8, 4):
        b = hip.flow_tvl1_step(f, b, k=k)
    assert torch.equal(a, b)


def _frames(h, w, kind, seed=3):
    """(img1, img2, true flow (2, h, w)) with img1(x) = img2(x + flow(x))."""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    if kind == "translation":
        d = (1.7, -0.9)
        return R.synth_texture(h, w, seed), R.synth_texture(h, w, seed, dx=d[0], dy=d[1]), np.stack([np.full((h, w), d[0]), np.full((h, w), d[1])])
    if kind == "rotation_zoom":
        ang, zoom = 0.02, 1.015
        cx, cy = (w - 1) / 2, (h - 1) / 2
        A = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) * zoom
        Ai = np.linalg.inv(A)
        # img2(y) = T(A^-1 (y - c) + c)  =>  img2(A (x - c) + c) = T(x) = img1(x)
        X2 = Ai[0, 0] * (x - cx) + Ai[0, 1] * (y - cy) + cx
        Y2 = Ai[1, 0] * (x - cx) + Ai[1, 1] * (y - cy) + cy
        fx = A[0, 0] * (x - cx) + A[0, 1] * (y - cy) + cx - x
        fy = A[1, 0] * (x - cx) + A[1, 1] * (y - cy) + cy - y
        return R.synth_texture(h, w, seed), R.synth_texture(h, w, seed, field=(X2, Y2)), np.stack([fx, fy])
    # occluder: static background, a textured square moving by d
    d = (2.6, 1.4)
    s = h // 3
    y0, x0 = h // 3, w // 3
    bg = R.synth_texture(h, w, seed)
    fg1 = R.synth_texture(h, w, seed + 1)
    fg2 = R.synth_texture(h, w, seed + 1, dx=d[0], dy=d[1])
    in1 = (x >= x0) & (x < x0 + s) & (y >= y0) & (y < y0 + s)
    in2 = (x >= x0 + d[0]) & (x < x0 + s + d[0]) & (y >= y0 + d[1]) & (y < y0 + s + d[1])
    img1, img2 = np.where(in1[..., None], fg1, bg), np.where(in2[..., None], fg2, bg)
    return img1, img2, np.stack([np.where(in1, d[0], 0.0), np.where(in1, d[1], 0.0)])


def _epe(f, true):
    f = f.double().cpu().numpy() if torch.is_tensor(f) else f
    return float(np.sqrt(((f - true) ** 2).sum(0)).mean())


@pytest.mark.parametrize("hw", [(40, 48), (33, 70)])
def test_whole_estimate_against_fp64_restatement(stream, hw):
    """The bar is the fp32 restatement's own distance from fp64 (same scheme, same operation order, torch on the host) times 3:
    measured on one MI355X, GPU vs fp64 3.6e-6 / 3.0e-6 and fp32 CPU vs fp64 3.7e-6 / 2.5e-6 (rel-L2) at 40 x 48 / 33 x 70."""
    import hip
    h, w = hw
    img1, img2, _ = _frames(h, w, "rotation_zoom")
    lv = hip.flow_levels(h, w, 5)
    want = R.estimate(img1, img2, dtype=torch.float64)
    cpu32 = R.estimate(img1, img2, dtype=torch.float32)
    a, b = torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda()
    single = hip.flow_tvl1(a, b, lv, 5, 100, 0)
    blocked = hip.flow_tvl1(a, b, lv, 5, 100, 8)
    assert torch.equal(single, blocked)
    e_gpu, e_cpu = rel_l2(single.cpu(), want), rel_l2(cpu32, want)
    print(f"{h}x{w}: gpu vs fp64 {e_gpu:.3e}, fp32 cpu vs fp64 {e_cpu:.3e}")
    assert e_gpu <= 3 * e_cpu + 1e-7


@pytest.mark.parametrize("size", [256, 1024])
@pytest.mark.parametrize("kind", ["translation", "rotation_zoom", "occluder"])
def test_end_point_error_on_synthetic_scenes(stream, size, kind):
    """Mean end-point error of the estimate on synthetic scenes, against the fp64 oracle (tests/flow_restatement.py run in fp64 on
    the device) on the same frames: no worse than the oracle's + 0.005 px.  Measured on one MI355X (GPU = oracle to 1e-4 px in every
    case): translation 0.0083 / 0.0062 px, rotation + zoom 0.083 / 0.179 px, occluder 0.021 / 0.0057 px at 256^2 / 1024^2.  And
    absolute bounds away from the frame edge, where the scene is well posed."""
    import flow
    img1, img2, true = _frames(size, size, kind)
    got = flow.estimate_tvl1(img1, img2).transpose(2, 0, 1)
    oracle = R.estimate(img1, img2, dtype=torch.float64, device="cuda")
    e, eo = _epe(got, true), _epe(oracle, true)
    print(f"{kind} {size}: EPE {e:.4f} px, oracle {eo:.4f} px")
    assert e <= eo + 0.005
    m = 24  # away from the frame edge (data enter or leave the frame there)
    assert _epe(got[:, m:-m, m:-m], true[:, m:-m, m:-m]) <= {"translation": 0.05, "rotation_zoom": 0.15, "occluder": 0.6}[kind]


def test_mask_is_pixel_identical_to_the_reference(stream):
    import flow
    for i, c in enumerate(R.fixture_cases(os.path.join(GOLDEN, "flow_consistency.npz"))):
        got = flow.check_consistency(c["flow1"], c["flow2"])
        assert got.dtype == np.uint8 and got.shape == c["mask"].shape
        assert (got == c["mask"]).all(), (i, c["kind"], int((got != c["mask"]).sum()))


def test_rerun_and_graph_replay_are_bit_identical(stream):
    import hip
    h, w = 72, 100
    img1, img2, _ = _frames(h, w, "occluder")
    a, b = torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda()
    lv = hip.flow_levels(h, w)
    ws = torch.empty(hip.flow_tvl1_workspace_bytes(h, w, lv), dtype=torch.uint8, device="cuda")
    first = hip.flow_tvl1(a, b, lv, 5, 100, 8, workspace=ws).clone()
    again = hip.flow_tvl1(a, b, lv, 5, 100, 8, workspace=ws).clone()
    assert torch.equal(first, again)
    out = torch.empty(2, h, w, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.flow_tvl1(a, b, lv, 5, 100, 8, out=out, workspace=ws)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    f1 = first.contiguous()
    f2 = hip.flow_tvl1(b, a, lv, 5, 100, 8, workspace=ws).clone()
    m = [hip.flow_consistency(f1, f2).clone() for _ in range(2)]
    assert torch.equal(m[0], m[1])


def test_largest_frame_runs(stream):
    """A 4096 x 2160 pair: every kernel at the size where 32-bit pixel offsets of the 6-plane state would overflow."""
    import flow
    h, w = 2160, 4096
    img1, img2, _ = _frames(h, w, "translation")
    f12 = flow.estimate_tvl1(img1, img2)
    assert f12.shape == (h, w, 2) and np.isfinite(f12).all()
    inner = f12[200:-200, 200:-200]
    assert abs(float(inner[..., 0].mean()) - 1.7) < 0.05 and abs(float(inner[..., 1].mean()) + 0.9) < 0.05
    f21 = flow.estimate_tvl1(img2, img1)
    m = flow.check_consistency(f12, f21)
    assert m.shape == (h, w) and 0.3 < float((m == 0).mean()) < 1.0


def _style(argv, cwd):
    env = dict(os.environ, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "style.py")] + argv, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=1200)


def test_vid_img_tvl1_end_to_end(tmp_path, weight_files):
    """style.py --transfer_type vid_img --flow_models tvl1 on 3 moving frames writes the whole flow cache, then runs the temporal
    loop; a second run that finds that cache in place estimates nothing and writes the same frames."""
    from PIL import Image
    clip = tmp_path / "clip"
    clip.mkdir()
    for i in range(3):
        Image.fromarray(R.synth_texture(56, 64, 9, dx=1.5 * i, dy=-0.5 * i)).save(clip / f"{i:05d}.png")
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    argv = ["--transfer_type", "vid_img", "--content", str(clip), "--style", os.path.join(REPO, "tests", "synth_style_256.png"),
            "--flow_models", "tvl1", "--image_sizes", "48", "--num_iters", "4", "--passes_per_scale", "2", "--init", "prev_warp",
            "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args", str(scaling), "--seed", "0", "--no_hist_match"]
    out1, out2 = tmp_path / "out1", tmp_path / "out2"
    r = _style(argv + ["--output_dir", str(out1)], cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    fdir = out1 / "clip_synth_style_256" / "flow"
    names = [f"{i:05d}" for i in range(3)]
    want = set()
    for a, b in zip(names, names[1:] + names[:1]):
        want |= {f"forward_{a}_{b}.flo", f"backward_{b}_{a}.flo", f"forward_{a}_{b}.png", f"backward_{b}_{a}.png"}
    assert set(os.listdir(fdir)) == want
    assert r.stdout.count("processed optical flow") == 3
    shutil.copytree(fdir, out2 / "clip_synth_style_256" / "flow")
    stamps = {f: os.path.getmtime(out2 / "clip_synth_style_256" / "flow" / f) for f in want}
    r2 = _style(argv + ["--output_dir", str(out2)], cwd=PKG)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "processed optical flow" not in r2.stdout
    assert stamps == {f: os.path.getmtime(out2 / "clip_synth_style_256" / "flow" / f) for f in want}
    frames1 = sorted(os.listdir(out1 / "clip_synth_style_256" / "48"))
    assert frames1 == sorted(f"{p}_{n}.png" for p in (1, 2) for n in names)
    for f in frames1:
        a = np.asarray(Image.open(out1 / "clip_synth_style_256" / "48" / f))
        b = np.asarray(Image.open(out2 / "clip_synth_style_256" / "48" / f))
        assert (a == b).all(), f
