"""Neural cellular automaton, host side: the fp64 restatement (perception against torch's circular pad + conv2d, its backward
against central differences), the pinned update-mask function, schedules, the CLI, checkpoints (including the reference's
whole-module pickles) and the invalid-argument paths of the new C-ABI entries.  No GPU needed."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nca_restatement as R
from conftest import PKG, REPO


def _params(chn, hidden, seed, w2_scale=0.1):
    rng = np.random.default_rng(seed)
    k = 4 * chn
    return np.concatenate([rng.normal(0, 0.2, hidden * k), rng.normal(0, 0.1, hidden), rng.normal(0, w2_scale, chn * hidden)])


def test_perception_is_circular_channel_major():
    """Restated perception = torch's circular pad 1 + conv2d of every channel with the stacked filters, reshaped (b, 4c, h, w)."""
    rng = np.random.default_rng(0)
    for b, c, h, w in ((2, 3, 5, 7), (1, 12, 1, 1), (1, 2, 2, 3)):
        x = rng.normal(size=(b, c, h, w))
        t = torch.from_numpy(x).reshape(b * c, 1, h, w)
        want = F.conv2d(F.pad(t, [1, 1, 1, 1], "circular"), torch.from_numpy(R.FILTERS)[:, None]).reshape(b, 4 * c, h, w)
        np.testing.assert_allclose(R.perceive(x), want.numpy(), rtol=0, atol=1e-12)


def test_perception_adjoint():
    rng = np.random.default_rng(1)
    x, d = rng.normal(size=(2, 3, 4, 6)), rng.normal(size=(2, 12, 4, 6))
    assert abs(np.sum(R.perceive(x) * d) - np.sum(x * R.perceive_t(d, 3))) < 1e-10


@pytest.mark.parametrize("steps", [1, 8])
def test_backward_matches_central_differences(steps):
    chn, hidden, h, w = 12, 96, 5, 6
    rng = np.random.default_rng(2)
    params = _params(chn, hidden, 3)
    x0 = rng.normal(0, 0.5, (2, chn, h, w))
    masks = [R.mask(7, s, 2, h, w) for s in range(steps)]
    gl = rng.normal(size=x0.shape)

    def loss(x, p):
        for m in masks:
            x = R.step(x, p, chn, hidden, m)
        return float(np.sum(x * gl))

    dx0, dp = R.chain_bwd(x0, gl, params, chn, hidden, masks)
    eps = 1e-6
    for idx in [(0, 0, 0, 0), (1, 5, 4, 5), (0, 11, 2, 3)]:
        e = np.zeros_like(x0)
        e[idx] = eps
        fd = (loss(x0 + e, params) - loss(x0 - e, params)) / (2 * eps)
        assert abs(fd - dx0[idx]) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, dx0[idx])
    for i in [0, 47, 100, hidden * 48 + 3, hidden * 48 + hidden + 17, len(params) - 1]:
        e = np.zeros_like(params)
        e[i] = eps
        fd = (loss(x0, params + e) - loss(x0, params - e)) / (2 * eps)
        assert abs(fd - dp[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, dp[i])


# ---- what the element-wise backward comparison of tests/test_nca_bwd_gpu.py stands on ---------------------------------------------
def _preact(x, params, chn, hidden):
    w1, b1, _ = R.split(params, chn, hidden, x.dtype)
    return np.einsum("jk,bkhw->bjhw", w1, R.perceive(x)) + b1[None, :, None, None]


@pytest.mark.parametrize("chn,hidden", R.PAIRS)
def test_zeroed_gradient_makes_the_backward_independent_of_near_tie_decisions(chn, hidden):
    """With g = 0 on the near_tie pixels, flipping every hidden unit's ReLU decision at every flagged pixel changes no output."""
    n, h, w = 2, 19, 23
    params = R.case_params(chn, hidden, 1)
    x, g = (a.astype(np.float64) for a in R.case_state(chn, n, h, w))
    m, _ = R.case_mask(n, h, w, "ones")
    tie = R.near_tie(x, params, chn, hidden)
    assert tie.any() and tie.mean() <= R.TIE_SHARE
    flipped = (_preact(x, params, chn, hidden) > 0) ^ tie[:, None]
    g0 = g * ~tie[:, None]
    want = R.step_bwd(x, g0, params, chn, hidden, m)
    got = R.step_bwd(x, g0, params, chn, hidden, m, relu=flipped)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for a, b in zip(R.step_bwd_abs(x, g0, params, chn, hidden, m, relu=flipped), R.step_bwd_abs(x, g0, params, chn, hidden, m)):
        assert np.array_equal(a, b)
    # and the zeroing is what does it: with g left alone the flipped decisions move dx
    assert not np.array_equal(R.step_bwd(x, g, params, chn, hidden, m, relu=flipped)[0], R.step_bwd(x, g, params, chn, hidden, m)[0])


def test_near_tie_share_of_every_backward_case():
    """The condition of the element-wise GPU cases: at most 2 % of the pixels lose their gradient, for every (pair, shape)."""
    cases = R.bwd_cases()
    assert {c[2:5] for c in cases} >= {R.SLOT_SHAPE, R.CHAIN_SHAPE, R.EXTREME_SHAPE} | set(R.MASK_SHAPES) | set(R.PLAN_SHAPES)
    seen = {}
    for chn, hidden, n, h, w, _ in cases:
        if (chn, n, h, w) not in seen:
            x = R.case_state(chn, n, h, w)[0].astype(np.float64)
            seen[chn, n, h, w] = float(R.near_tie(x, R.case_params(chn, hidden, 1), chn, hidden).mean())
    assert max(seen.values()) <= R.TIE_SHARE, {k: v for k, v in seen.items() if v > R.TIE_SHARE}
    assert seen[12, 4, 160, 160] > 0 and seen[16, 3, 150, 170] > 0  # (the flagged set is not empty where it matters)


@pytest.mark.parametrize("chn,hidden,n,h,w,mode", [(12, 96, 2, 19, 23, "rate0.5"), (16, 128, 1, 5, 13, "ones"), (12, 96, 3, 2, 1, "given"),
                                                   (16, 128, 1, 1, 1, "ones")])
def test_abs_backward_bounds_the_backward(chn, hidden, n, h, w, mode):
    params = R.case_params(chn, hidden, 1)
    x, g = (a.astype(np.float64) for a in R.case_state(chn, n, h, w))
    m, _ = R.case_mask(n, h, w, mode)
    for v, a in zip(R.step_bwd(x, g, params, chn, hidden, m), R.step_bwd_abs(x, g, params, chn, hidden, m)):
        assert v.shape == a.shape and np.all(a >= 0) and np.all(np.abs(v) <= a * (1 + 1e-12))


@pytest.mark.parametrize("chn,hidden", R.PAIRS)
def test_near_tie_scale_dominates_the_fp32_error_of_the_preactivation(chn, hidden):
    """|a32 - a64| <= 5e-6 S everywhere (the derivation in near_tie's docstring gives 4.1e-6 S for any evaluation order): half of
    near_tie's tolerance, so an fp32 decision outside the flagged set is the fp64 decision."""
    params = R.case_params(chn, hidden, 1)
    x = R.case_state(chn, 3, 150, 170)[0]
    a32 = _preact(x, params, chn, hidden)
    assert a32.dtype == np.float32
    a64 = _preact(x.astype(np.float64), params, chn, hidden)
    S = R.preact_scale(x.astype(np.float64), params, chn, hidden)[1]
    assert np.all(np.abs(a32 - a64) <= 5e-6 * S), float(np.max(np.abs(a32 - a64) / S))
    tie = R.near_tie(x.astype(np.float64), params, chn, hidden)
    assert np.array_equal((a32 > 0)[~np.broadcast_to(tie[:, None], a32.shape)], (a64 > 0)[~np.broadcast_to(tie[:, None], a32.shape)])


def test_restatement_follows_the_dtype_of_the_state():
    """The fp32 twin of the folded-chain test: the same functions on fp32 arrays stay in fp32 and land near the fp64 result."""
    chn, hidden, n, h, w = 12, 96, 2, 9, 11
    params = R.case_params(chn, hidden, 4, w2_scale=0.01, w1_scale=0.03)
    x, g = R.case_state(chn, n, h, w)
    masks = [R.mask(5, k, n, h, w) for k in range(3)]
    d32, p32 = R.chain_bwd(x, g, params, chn, hidden, masks)
    d64, p64 = R.chain_bwd(x.astype(np.float64), g.astype(np.float64), params, chn, hidden, masks)
    assert d32.dtype == p32.dtype == np.float32 and d64.dtype == p64.dtype == np.float64
    assert 0 < np.linalg.norm(d32 - d64) <= 1e-5 * np.linalg.norm(d64) and 0 < np.linalg.norm(p32 - p64) <= 1e-4 * np.linalg.norm(p64)


def _splitmix_scalar(z):
    z = (z + 0x9E3779B97F4A7C15) & R.M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & R.M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & R.M64
    return z ^ (z >> 31)


def _u24(seed, step, b, y, x):
    """DESIGN.md's statement of the mask function with Python integers: 2^24 u."""
    key = _splitmix_scalar(seed ^ _splitmix_scalar(step))
    return _splitmix_scalar(key ^ ((b << 40) | (y << 20) | x)) >> 40


def test_mask_function_is_pinned():
    u = R.mask_u(1, 5, 3, 4, 5)
    assert u.dtype == np.float32 and np.all(u >= 0) and np.all(u < 1)
    for b, y, x in ((0, 0, 0), (2, 3, 4), (1, 2, 0)):
        assert int(u[b, y, x] * 2 ** 24) == _u24(1, 5, b, y, x)
    assert int(R.mask_u(2 ** 64 - 1, 123456, 1, 1, 2)[0, 0, 1] * 2 ** 24) == _u24(2 ** 64 - 1, 123456, 0, 0, 1)
    # hard-coded values, so that the function cannot drift
    assert [_u24(0, 0, 0, 0, 0), _u24(1, 5, 2, 3, 4), _u24(2 ** 64 - 1, 123456, 0, 0, 1)] == PINNED
    m = R.mask(42, 3, 4, 128, 128)
    assert set(np.unique(m)) == {0.0, 1.0} and abs(float(m.mean()) - 0.5) < 0.01
    rm = np.full((64, 64), 0.25, np.float32)
    assert abs(float(R.mask(1, 1, 4, 64, 64, rate_map=rm).mean()) - 0.25) < 0.02
    assert not np.array_equal(R.mask(1, 1, 1, 32, 32), R.mask(1, 2, 1, 32, 32))


PINNED = [2327157, 7762653, 12357813]


def test_schedules():
    import nca
    for i in (0, 1, 1999, 2000, 3999, 4000, 7499):
        assert nca.lr_at(i) == pytest.approx(R.lr(i), rel=1e-15)
    assert [nca.evolution_steps(k) for k in (0, 29, 30, 60, 149, 150, 599)] == [1, 1, 2, 4, 16, 32, 32]
    assert all(nca.evolution_steps(k) == R.evolution_steps(k) and nca.rate_map_steps(k) == R.rate_map_steps(k) for k in range(600))
    assert nca.rate_map_steps(0) == 1 and nca.rate_map_steps(31) == 2 and nca.rate_map_steps(599) == 32
    assert nca.fade(400) == 1.0 and nca.fade(450) == 0.5 and nca.fade(0) == 1.0
    assert [i for i in range(100) if R.seeded(i)] == [0, 32, 64, 96]
    assert nca.SEED_EVERY == 32 and nca.STEP_N_RANGE == (32, 96) and nca.STYLE_LAYERS == [1, 6, 11, 18, 25]


def test_batch_mean_gram_loss_restatement_matches_torch():
    rng = np.random.default_rng(4)
    feats = [rng.normal(size=(3, 4, 5, 6)), rng.normal(size=(3, 2, 3, 3))]
    tg = [rng.normal(size=(4, 4)), rng.normal(size=(2, 2))]
    want = 0.0
    for f, t in zip(feats, tg):
        ft = torch.from_numpy(f)
        g = torch.einsum("bchw,bdhw->bcd", ft, ft) / (f.shape[2] * f.shape[3])
        want += float((g.mean(0) - torch.from_numpy(t)).square().mean())
    assert R.batch_mean_gram_loss(feats, tg) == pytest.approx(want, rel=1e-12)


def test_cli_defaults_and_parsing():
    import nca
    a = nca.parse_args(["train", "s.png", "out"])
    assert (a.cmd, a.style, a.out_dir, a.vgg_file, a.steps, a.seed, a.batch, a.pool) == \
        ("train", "s.png", "out", "modelzoo/vgg16-397923af.pth", 7500, 0, 4, 1024, )
    assert (a.size, a.chn, a.hidden, a.checkpoint_every) == (128, 12, 96, 500)
    r = nca.parse_args(["render", "s.png", "out"])
    assert (r.checkpoint, r.frames, r.size, r.rate_map, r.checkgrid) == (None, 600, 256, None, False)
    r = nca.parse_args(["render", "s.png", "out", "--checkpoint", "c.pt", "--frames", "3", "--size", "64", "--rate_map", "t.png",
                        "--checkgrid"])
    assert (r.checkpoint, r.frames, r.size, r.rate_map, r.checkgrid) == ("c.pt", 3, 64, "t.png", True)
    with pytest.raises(SystemExit):
        nca.parse_args(["paint", "s.png", "out"])


def test_missing_vgg_file_is_an_error_not_a_download(tmp_path):
    import nca
    with pytest.raises(FileNotFoundError, match="never downloads"):
        nca.StyleModel(str(tmp_path / "vgg16-397923af.pth"), "cpu")


def test_checkpoint_round_trip(tmp_path):
    import nca
    ca = nca.NCA.init(16, 128, seed=3, device="cpu")
    ca.params[-5:] = torch.arange(5.0)
    f = str(tmp_path / "style_500.pt")
    nca.save_checkpoint(ca, f)
    sd = torch.load(f, weights_only=True)
    assert sd["chn"] == 16 and sd["hidden"] == 128 and tuple(sd["w1.weight"].shape) == (128, 64, 1, 1)
    back = nca.load_checkpoint(f, device="cpu")
    assert (back.chn, back.hidden) == (16, 128) and torch.equal(back.params, ca.params)


class CA(torch.nn.Module):
    """Shaped like the reference's CA (NCA_train.py:165-173); torch.save of the whole module is what its checkpoints hold."""

    def __init__(self, chn=12, hidden_n=96):
        super().__init__()
        self.chn = chn
        self.w1 = torch.nn.Conv2d(chn * 4, hidden_n, 1)
        self.w2 = torch.nn.Conv2d(hidden_n, chn, 1, bias=False)


def test_reads_whole_module_pickles(tmp_path):
    import nca
    torch.manual_seed(0)
    ca = CA()
    with torch.no_grad():
        ca.w2.weight.normal_()
    f = str(tmp_path / "style_7500.pt")
    torch.save(ca, f)
    got = nca.load_checkpoint(f, device="cpu")
    w1, b1, w2 = got.tensors()
    assert got.chn == 12 and got.hidden == 96
    assert torch.equal(w1, ca.w1.weight[:, :, 0, 0]) and torch.equal(b1, ca.w1.bias) and torch.equal(w2, ca.w2.weight[:, :, 0, 0])


class _Payload:
    def __reduce__(self):
        return (os.system, ("true",))


def test_restricted_unpickler_refuses_other_globals(tmp_path):
    import nca
    f = str(tmp_path / "evil.pt")
    torch.save({"w1.weight": _Payload()}, f)
    with pytest.raises(pickle.UnpicklingError):
        nca.load_checkpoint(f, device="cpu")
    torch.save([torch.zeros(1)], f)
    with pytest.raises(ValueError):
        nca.load_checkpoint(f, device="cpu")


def test_style_image_reading(tmp_path):
    import nca
    from PIL import Image
    g = str(tmp_path / "grey.png")
    Image.fromarray(np.uint8(np.arange(300 * 200).reshape(200, 300) % 256)).save(g)
    a = nca.imread_style(g)
    assert a.shape == (85, 128, 3) and a.dtype == np.float32 and 0 <= a.min() and a.max() <= 1
    a = nca.imread_style(os.path.join(REPO, "tests", "synth_style_256.png"))
    assert a.shape == (128, 128, 3)


def test_invalid_arguments_are_rejected_without_a_gpu():
    import hip
    L = hip.lib()
    P = 0x10000
    assert L.maua_nca_supported(1, 12, 96, 4096, 4096) == 1 and L.maua_nca_supported(4, 16, 128, 128, 128) == 1
    assert L.maua_nca_supported(1, 12, 128, 8, 8) == 0 and L.maua_nca_supported(0, 12, 96, 8, 8) == 0
    assert L.maua_nca_supported(1, 12, 96, 1 << 15, 1 << 15) == 0 and L.maua_nca_supported(1, 12, 96, -1, 8) == 0
    assert L.maua_nca_param_count(12, 96) == 96 * 48 + 96 + 12 * 96 and L.maua_nca_param_count(16, 128) == 128 * 64 + 128 + 16 * 128
    assert L.maua_nca_param_count(12, 97) == 0
    assert L.maua_nca_step(None, P, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_nca_step(P, P, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, 0, None) == -1  # out aliases x
    assert L.maua_nca_step(P, P + 64, P, 1, 12, 64, 8, 8, 0.5, None, None, 0, 0, None) == -2
    assert L.maua_nca_step(P, P + 64, P, 1, 12, 96, 0, 8, 0.5, None, None, 0, 0, None) == -1
    assert L.maua_nca_step(P, P + 64, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, -1, None) == -1
    assert L.maua_nca_bwd_workspace_bytes(4, 12, 96, 128, 128) >= 4 * 48 * 128 * 128 * 4
    assert L.maua_nca_bwd_workspace_bytes(4, 12, 95, 128, 128) == 0 and L.maua_nca_bwd_workspace_bytes(-4, 12, 96, 128, 128) == 0
    need = L.maua_nca_bwd_workspace_bytes(1, 12, 96, 8, 8)
    assert L.maua_nca_step_bwd(P, P + 64, P + 128, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, 0, 1, P, need - 1, None) == -3
    assert L.maua_nca_step_bwd(P, P + 64, P, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, 0, 1, P, need, None) == -1  # dx aliases x
    assert L.maua_nca_step_bwd(P, P + 64, P + 128, P, 1, 12, 96, 8, 8, 0.5, None, None, 0, 0, 1, None, need, None) == -1
    assert L.maua_nca_grad_finish(P, 1, 12, 96, 8, 8, P, need - 1, 1, None) == -3
    assert L.maua_nca_grad_finish(None, 1, 12, 96, 8, 8, P, need, 1, None) == -1
    assert L.maua_nca_grad_finish(P, 1, 16, 96, 8, 8, P, need, 1, None) == -2


def test_host_boundary_fuzz_under_sanitizers():
    """The new entry points' host half (argument checks, workspace sizing) under the ASan/UBSan build, with extents up to INT_MAX."""
    import build_native
    asan = build_native.asan_runtime()
    if asan is None:
        pytest.skip("clang's asan runtime not found")
    lib = build_native.build(sanitize=True)
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz_nca_host.py"), lib, "3000", "0"], capture_output=True,
                         text=True, env=env, timeout=600, cwd="/tmp")
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert "no sanitizer report" in out.stdout and "runtime error" not in out.stderr
