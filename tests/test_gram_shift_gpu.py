"""The shifted Gram kernels (csrc/gram_shift.hip) against fp64 (tests/shift_restatement.py) at the bar of the guided kernel tests: TOL =
2e-5, the project's bar for contractions, relative L2.

Shapes (C, H, W) and what they cross: (3, 5, 7) - 15 and 7 valid pairs, less than one 64-pixel stage; (70, 9, 33) - the plane (297) ends
inside a stage, row ends walk through the stages, a ragged channel tile; (130, 20, 35) - the y offset 16 x 35 = 560 exceeds the backward
kernel's 256-pixel tile, three channel tiles, one ragged; (64, 16, 64) and (128, 32, 32) - aligned rows; (64, 64, 128) - relu1_1 of a 128-pixel
job with its four shifts.  Every shape runs with and without row means."""
import ctypes

import pytest
import torch

import shift_restatement as sr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
X, Y = 0, 1
SHAPES = {
    (3, 5, 7): [(X, 4), (Y, 4)],
    (70, 9, 33): [(X, 4), (X, 16), (Y, 4)],
    (130, 20, 35): [(X, 4), (Y, 4), (X, 16), (Y, 16)],
    (64, 16, 64): [(X, 4), (Y, 4)],
    (128, 32, 32): [(X, 4), (Y, 4)],
    (64, 64, 128): [(X, 4), (Y, 4), (X, 16), (Y, 16)],
}
CASES = [(shape, cov) for shape in SHAPES for cov in (False, True)]
IDS = [f"{'x'.join(map(str, s))}-{'centred' if c else 'plain'}" for s, c in CASES]


def feature_map(shape):
    g = torch.Generator().manual_seed(17 + sum(shape))
    return torch.relu(torch.randn(*shape, generator=g) + 0.3), g


def scales_of(shape, shifts):
    C, H, W = shape
    return [1.0 / (C * (H * (W - d) if a == X else (H - d) * W)) for a, d in shifts]


@pytest.fixture(scope="module")
def references():
    """fp64 matrices and gradients per case, computed once."""
    out = {}
    for shape, cov in CASES:
        f, g = feature_map(shape)
        shifts = SHAPES[shape]
        f64 = f.double()
        grams = torch.stack([sr.shifted_gram(f64, a, d, cov) for a, d in shifts])
        d = torch.randn(len(shifts), shape[0], shape[0], generator=g)  # not symmetric
        x64 = f64 - f64.mean((1, 2), keepdim=True) if cov else f64
        gx = sr.shift_backward(x64, shifts, [m.double() for m in d], False)  # dL/dX: the term through the means is the caller's
        base = torch.randn(*shape, generator=g) * float(gx.abs().max())
        out[(shape, cov)] = dict(f=f, grams=grams, d=d, gx=gx, base=base)
    return out


@pytest.mark.parametrize("shape,cov", CASES, ids=IDS)
def test_forward_and_backward_against_fp64(references, shape, cov):
    import hip
    ref = references[(shape, cov)]
    shifts, sc = SHAPES[shape], scales_of(shape, SHAPES[shape])
    f = ref["f"].cuda()
    mean = f.double().mean((1, 2)).float().contiguous() if cov else None
    assert hip.gram_shift_supported(len(shifts), *shape)
    got = hip.gram_shift_fwd(f, shifts, sc, mean)
    again = hip.gram_shift_fwd(f, shifts, sc, mean)
    torch.cuda.synchronize()
    for s, (a, d) in enumerate(shifts):
        e = rel_l2(got[s].cpu(), ref["grams"][s])
        print(f"  G[{'xy'[a]}{d}]: rel-L2 {e:.3e}")
        assert e <= TOL, (a, d, e)
    assert torch.equal(got, again)  # two calls, equal bits
    dm = ref["d"].cuda()
    gx = torch.full(shape, float("nan"), device="cuda")
    hip.gram_shift_bwd(dm, f, shifts, sc, mean, gx, False)
    acc = ref["base"].cuda().clone()
    hip.gram_shift_bwd(dm, f, shifts, sc, mean, acc, True)
    gx2 = torch.empty(shape, device="cuda")
    hip.gram_shift_bwd(dm, f, shifts, sc, mean, gx2, False)
    torch.cuda.synchronize()
    e0, e1 = rel_l2(gx.cpu(), ref["gx"]), rel_l2(acc.cpu().double() - ref["base"].double(), ref["gx"])
    print(f"  gx: rel-L2 {e0:.3e}, accumulated {e1:.3e}")
    assert e0 <= TOL and e1 <= TOL
    assert torch.equal(gx, gx2)


def test_a_shift_alone_has_the_bits_it_has_among_four():
    import hip
    shape = (130, 20, 35)
    shifts, sc = SHAPES[shape], scales_of(shape, SHAPES[shape])
    f = feature_map(shape)[0].cuda()
    mean = f.mean((1, 2)).contiguous()
    for mu in (None, mean):
        four = hip.gram_shift_fwd(f, shifts, sc, mu)
        for s in range(4):
            alone = hip.gram_shift_fwd(f, shifts[s:s + 1], sc[s:s + 1], mu)
            assert torch.equal(alone[0], four[s]), shifts[s]


@pytest.mark.parametrize("shape", [(70, 9, 33), (64, 16, 64)], ids=["70x9x33", "64x16x64"])
def test_x_shift_equals_y_shift_of_the_transposed_map(shape):
    import hip
    C, H, W = shape
    f = feature_map(shape)[0].cuda()
    ft = f.transpose(1, 2).contiguous()
    gx = hip.gram_shift_fwd(f, [(X, 4)], [1.0 / (C * H * (W - 4))])
    gy = hip.gram_shift_fwd(ft, [(Y, 4)], [1.0 / (C * H * (W - 4))])
    e = rel_l2(gx.cpu(), gy.cpu().double())
    print(f"  rel-L2 {e:.3e}")
    assert e <= TOL
    assert rel_l2(gx[0].cpu(), gx[0].t().cpu().double()) > 1e-3  # (not symmetric: the check above is not vacuous)


def test_a_refused_delta_returns_the_error_and_leaves_gram_unwritten():
    import hip
    C, H, W = 3, 5, 7
    f = feature_map((C, H, W))[0].cuda()
    for axis, delta in ((X, 7), (Y, 5), (X, 0)):
        out = torch.full((2, C, C), 7.0, device="cuda")
        with pytest.raises(hip.HipError, match="shift"):
            hip.gram_shift_fwd(f, [(X, 4), (axis, delta)], [1.0, 1.0], out=out)
        gx = torch.full((C, H, W), 7.0, device="cuda")
        with pytest.raises(hip.HipError, match="shift"):
            hip.gram_shift_bwd(torch.zeros(2, C, C, device="cuda"), f, [(X, 4), (axis, delta)], [1.0, 1.0], None, gx, False)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((gx == 7.0).all())
    L = hip.lib()
    one, axes, deltas = (ctypes.c_double * 1)(1.0), (ctypes.c_int * 1)(X), (ctypes.c_int * 1)(7)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, C, C, device="cuda")
    assert L.maua_gram_shift_fwd(f.data_ptr(), None, axes, deltas, one, out.data_ptr(), 1, C, H, W, ws.data_ptr(), ws.numel(), None) == -2


def test_gram_matrix_module_returns_the_raw_shifted_product():
    import loss
    shape = (70, 9, 33)
    f, _ = feature_map(shape)
    x = f.cuda()[None].requires_grad_(True)
    g = loss.GramMatrix()
    for kw, (axis, d) in ((dict(shift_x=4), (X, 4)), (dict(shift_y=4, use_covariance=True), (Y, 4))):
        cov = bool(kw.get("use_covariance"))
        got = g(x, **kw)
        want = sr.shifted_gram(f.double(), axis, d, cov, normalise=False)
        assert got.shape == (70, 70) and rel_l2(got.detach().cpu(), want) <= TOL
        w = torch.randn(70, 70, generator=torch.Generator().manual_seed(5))
        x.grad = None
        (got * w.cuda()).sum().backward()
        f64 = f.double().requires_grad_(True)
        (sr.shifted_gram(f64, axis, d, cov, normalise=False) * w.double()).sum().backward()
        assert rel_l2(x.grad[0].cpu(), f64.grad) <= TOL
