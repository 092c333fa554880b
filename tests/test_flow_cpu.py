"""Optical flow for vid_img (--flow_models tvl1), host side: the fp64 restatement of the TV-L1 scheme, the restated reliability mask
against the reference's own (tests/golden/flow_consistency.npz, tools/make_flow_golden.py), the flow cache writer and the routing
in style.vid_img with a stub estimator, and the new C-ABI entries.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import flow_restatement as R
from conftest import GOLDEN, REPO

FIXTURE = os.path.join(GOLDEN, "flow_consistency.npz")


@pytest.mark.parametrize("d", [(1.3, -0.6), (-0.45, 0.8)])
def test_fp64_restatement_recovers_a_subpixel_translation(d):
    """img2 = img1 moved by d, so img1(x) = img2(x + d): the estimate is +d (sign included) away from the frame edges."""
    a = R.synth_texture(64, 80, 1)
    b = R.synth_texture(64, 80, 1, dx=d[0], dy=d[1])
    f = R.estimate(a, b, iters=60)
    inner = f[:, 16:-16, 16:-16]
    assert abs(float(inner[0].mean()) - d[0]) < 0.03 and abs(float(inner[1].mean()) - d[1]) < 0.03, inner.mean((1, 2))
    assert float((inner[0] - d[0]).abs().max()) < 0.25 and float((inner[1] - d[1]).abs().max()) < 0.25


def test_restatement_steps_keep_the_boundary_rules():
    """div is the negative adjoint of the forward difference (zero on the last row / column): <grad u, p> = -<u, div p>."""
    g = torch.Generator().manual_seed(0)
    for h, w in ((1, 7), (5, 1), (6, 9)):
        u = torch.randn(h, w, generator=g, dtype=torch.float64)
        px, py = torch.randn(h, w, generator=g, dtype=torch.float64), torch.randn(h, w, generator=g, dtype=torch.float64)
        gx, gy = torch.zeros(h, w, dtype=torch.float64), torch.zeros(h, w, dtype=torch.float64)
        gx[:, :-1] = u[:, 1:] - u[:, :-1]
        gy[:-1] = u[1:] - u[:-1]
        # div through tv_step with zero fields / zero u: u_new = theta div p
        S = torch.stack([torch.zeros(h, w, dtype=torch.float64)] * 2 + [px, py, px, py])
        F = torch.zeros(3, h, w, dtype=torch.float64)
        div = R.tv_step(F, S)[0] / R.THETA
        assert abs(float((gx * px + gy * py).sum() + (u * div).sum())) < 1e-9


def test_erosion_characterisation_equals_scipy_integer_blur():
    """scipy's gaussian_filter of an int64 field keeps the dtype and truncates after each 1-D pass: for fields in {-1, 0, 1} the
    blurred and clipped result is exactly the 41 x 41 erosion of the '+1' set (windows clamped to the frame)."""
    import scipy.ndimage
    rng = np.random.default_rng(3)
    for t in range(40):
        h, w = (int(v) for v in rng.integers(2, 110, 2))
        p = [rng.uniform(0, 0.02), rng.uniform(0, 0.02)]
        a = rng.choice([-1, 0, 1], size=(h, w), p=[p[0], p[1], 1 - p[0] - p[1]]).astype(np.int64)
        want = scipy.ndimage.gaussian_filter(a, [5, 5]).clip(0, 1)
        assert want.dtype == np.int64
        assert (R.erode41(a) == want).all(), (t, h, w)


def test_fixture_masks_equal_the_restated_classification():
    cases = R.fixture_cases(FIXTURE)
    kinds = [c["kind"] for c in cases]
    assert len(kinds) >= 20 and {"translation", "occluder", "rotation_zoom", "leaving"} <= set(kinds)
    shapes = {c["flow1"].shape[:2] for c in cases}
    assert any(h == 2 or w == 2 for h, w in shapes) and any(h % 2 and w % 2 for h, w in shapes) and any(max(h, w) < 41 for h, w in shapes)
    reliable = []
    for i, c in enumerate(cases):
        assert (R.classify(c["flow1"], c["flow2"]) == c["cls"]).all(), (i, c["kind"])
        assert (R.mask_bytes(c["flow1"], c["flow2"]) == c["mask"]).all(), (i, c["kind"])
        reliable.append(float((c["mask"] == 0).mean()))
    assert max(reliable) > 0.5 and sum(r > 0.2 for r in reliable) >= 3  # both values cover much of several frames
    # every class occurs, -1 included, in several cases
    assert sum(int((c["cls"] == -1).sum()) > 100 for c in cases) >= 3 and all(any((c["cls"] == v).any() for c in cases) for v in (-1, 0, 1))


def test_flow_to_image_matches_the_reference():
    import flow
    for i, c in enumerate(R.fixture_cases(FIXTURE)):
        assert (flow.flow_to_image(c["flow1"].copy()) == c["color"]).all(), i


def test_get_flow_model_selects_tvl1_and_refuses_networks():
    import argparse
    import config
    import flow
    args = config.get_args(["--content", "c", "--style", "s.png", "--transfer_type", "vid_img", "--flow_models", "tvl1"])
    assert args.flow_models == "tvl1" and flow.uses_tvl1(args) and callable(flow.get_flow_model(args))
    for bad in ("tvl1,pwc", "unflow,pwc,spynet,liteflownet"):
        with pytest.raises(ValueError, match="weights"):
            flow.get_flow_model(argparse.Namespace(flow_models=bad))
    assert not flow.uses_tvl1(config.get_args(["--content", "c", "--style", "s.png"]))


def _clip(tmp_path, n=3, S=24):
    d = tmp_path / "clip"
    d.mkdir()
    for i in range(n):
        Image.fromarray(R.synth_texture(S, S + 4, 5, dx=i)).save(d / f"{i:04d}.png")
    return str(d)


def _args(tmp_path, content, *extra):
    import config
    return config.get_args(["--content", content, "--style", os.path.join(REPO, "tests", "synth_style_256.png"), "--transfer_type",
                            "vid_img", "--flow_models", "tvl1", "--output_dir", str(tmp_path / "out"), *extra])


@pytest.mark.parametrize("no_check_occlusion", [False, True])
def test_flow_cache_writer_names_wrap_pair_and_resume(tmp_path, monkeypatch, no_check_occlusion):
    import load
    import flow
    content = _clip(tmp_path)
    args = _args(tmp_path, content, *(["--no_check_occlusion"] if no_check_occlusion else []))
    calls = []

    def model(a, b):
        calls.append((a.shape, b.shape))
        assert a.dtype == np.uint8 and a.shape == (24, 28, 3)
        return np.full(a.shape[:2] + (2,), 0.25 * len(calls), np.float32)
    monkeypatch.setattr(flow, "check_consistency", R.mask_bytes)  # the device kernel's restatement (test_flow_gpu.py pins the kernel to it)
    frames = flow.write_flow_cache(model, args)
    fdir = flow.flow_dir(args)
    assert fdir.startswith(str(tmp_path / "out" / "clip_synth_style_256"))
    assert [os.path.basename(f) for f in frames] == ["0000.png", "0001.png", "0002.png"]
    want = set()
    for a, b in (("0000", "0001"), ("0001", "0002"), ("0002", "0000")):  # the last pair wraps around to the first frame
        want |= {f"forward_{a}_{b}.flo", f"backward_{b}_{a}.flo", f"forward_{a}_{b}.png", f"backward_{b}_{a}.png"}
    assert set(os.listdir(fdir)) == want and len(calls) == 6
    f = load.read_flo(os.path.join(fdir, "backward_0001_0000.flo"))
    assert f.shape == (24, 28, 2) and float(f[0, 0, 0]) == 0.5  # the second model call of the first pair
    png = np.asarray(Image.open(os.path.join(fdir, "forward_0000_0001.png")))
    assert png.dtype == np.uint8 and png.shape == (24, 28)
    if not no_check_occlusion:
        assert (png == 255).all()  # 24 x 28 frames: nothing survives the 41 x 41 erosion
    flow.write_flow_cache(model, args)
    assert len(calls) == 6  # resume: every backward PNG exists
    os.remove(os.path.join(fdir, "backward_0000_0002.png"))
    flow.write_flow_cache(model, args)
    assert len(calls) == 8 and set(os.listdir(fdir)) == want


def _routing(tmp_path, monkeypatch, rank, argv_extra=(), temporal=True):
    import dist
    import flow
    import style
    content = _clip(tmp_path)
    extra = list(argv_extra) + ([] if temporal else ["--temporal_weight", "0"])
    args = _args(tmp_path, content, *extra) if "--flow_models" not in extra else None
    if args is None:
        import config
        args = config.get_args(["--content", content, "--style", os.path.join(REPO, "tests", "synth_style_256.png"), "--transfer_type",
                                "vid_img", "--output_dir", str(tmp_path / "out"), *extra])
    seen = []

    class Done(Exception):
        pass

    def write(model, a):
        seen.append("write")
        os.makedirs(flow.flow_dir(a), exist_ok=True)
        open(os.path.join(flow.flow_dir(a), "forward_0000_0001.flo"), "wb").close()

    def shard(*a):
        seen.append("independent")
        raise Done()
    monkeypatch.setattr(dist, "init", lambda: (rank, rank, 2))
    monkeypatch.setattr(dist, "shard_range", shard)
    monkeypatch.setattr(flow, "write_flow_cache", write)
    monkeypatch.setattr(flow, "get_flow_model", lambda a: (seen.append("model"), None)[1])
    monkeypatch.setattr(style, "_vid_img_flow", lambda *a: seen.append("temporal"))
    monkeypatch.setattr(style.load, "process_style_images", lambda a: [])
    try:
        style.vid_img(args)
    except Done:
        pass
    return seen


def test_vid_img_routing_rank0_writes_cache_then_runs_the_temporal_loop(tmp_path, monkeypatch):
    assert _routing(tmp_path, monkeypatch, 0) == ["model", "write", "temporal"]


def test_vid_img_routing_other_ranks_return_at_once(tmp_path, monkeypatch):
    assert _routing(tmp_path, monkeypatch, 1) == []


def test_vid_img_default_flags_never_estimate(tmp_path, monkeypatch):
    assert _routing(tmp_path, monkeypatch, 0, argv_extra=["--flow_models", "unflow,pwc,spynet,liteflownet"]) == ["independent"]


def test_vid_img_tvl1_without_temporal_weight_never_estimates(tmp_path, monkeypatch):
    assert _routing(tmp_path, monkeypatch, 0, temporal=False) == ["independent"]


FLOW_SYMBOLS = ["maua_flow_levels", "maua_flow_grey_u8", "maua_flow_pyr_down", "maua_flow_warp_prep", "maua_flow_tvl1_step",
                "maua_flow_tvl1_blocked", "maua_flow_median5", "maua_flow_upsample", "maua_flow_consistency_workspace_bytes",
                "maua_flow_consistency", "maua_flow_tvl1_workspace_bytes", "maua_flow_tvl1"]


def test_flow_entries_declared_bound_and_exported():
    import subprocess
    import build_native
    import hip
    head = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    for s in FLOW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, head), s
        assert s in hip.SIGNATURES, s
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_native.build()], text=True)
    assert all(f" T {s}\n" in out for s in FLOW_SYMBOLS)
    assert hip.lib().maua_abi_version() == 2


def test_flow_host_helpers_match_the_library():
    import hip
    L = hip.lib()
    for h, w in ((1, 1), (15, 40), (16, 16), (31, 33), (32, 32), (2, 50), (1080, 1920), (2160, 4096), (65536, 4096)):
        for lv in range(0, 9):
            assert L.maua_flow_levels(h, w, lv) == hip.flow_levels(h, w, lv), (h, w, lv)
            assert L.maua_flow_tvl1_workspace_bytes(h, w, lv) == hip.flow_tvl1_workspace_bytes(h, w, lv), (h, w, lv)
    assert hip.flow_levels(1080, 1920) == 5 and hip.flow_levels(40, 500) == 2 and hip.flow_levels(15, 900) == 1
    assert L.maua_flow_consistency_workspace_bytes(1080, 1920) >= 2 * 1080 * 1920
    assert L.maua_flow_levels(0, 5, 5) == 0 and L.maua_flow_tvl1_workspace_bytes(64, 64, 9) == 0


def test_flow_entries_reject_bad_arguments_without_touching_the_gpu():
    import hip
    L = hip.lib()
    fake = 4096  # never dereferenced: every call below fails its argument check first
    assert L.maua_flow_grey_u8(None, fake, 4, 4, None) == -1
    assert L.maua_flow_pyr_down(fake, fake, 0, 4, None) == -1
    assert L.maua_flow_warp_prep(fake, fake, None, fake, 4, 4, None) == -1
    assert L.maua_flow_tvl1_step(fake, fake, fake, 4, 4, None) == -1  # state_in == state_out
    assert L.maua_flow_tvl1_blocked(fake, fake, fake + 64, 4, 4, 0, None) == -1
    assert L.maua_flow_tvl1_blocked(fake, fake, fake + 64, 4, 4, 17, None) == -1
    assert L.maua_flow_median5(fake, fake + 64, 4, 1 << 17, 1, None) == -1
    assert L.maua_flow_upsample(fake, 0, 3, fake, 4, 4, 2, 2.0, None) == -1
    assert L.maua_flow_consistency(fake, fake, fake, 1, 9, fake, 1 << 20, None) == -1  # sides >= 2
    assert L.maua_flow_consistency(fake, fake, fake, 9, 9, fake, 16, None) == -3      # workspace too small
    assert L.maua_flow_tvl1(fake, fake, fake, 64, 64, 9, 5, 100, 8, fake, 1 << 30, None) == -1
    assert L.maua_flow_tvl1(fake, fake, fake, 64, 64, 3, 5, 100, 17, fake, 1 << 30, None) == -1
    assert L.maua_flow_tvl1(fake, fake, fake, 64, 64, 3, 5, 100, 8, fake, 16, None) == -3
    assert b"workspace" in L.maua_last_error()
