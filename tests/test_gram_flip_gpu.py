"""The mirrored Gram kernels (csrc/gram_flip.hip) against fp64 (tests/flip_restatement.py) at the bar of the shifted kernel tests: TOL =
2e-5, the project's bar for contractions, relative L2.

Shapes (C, H, W) and what they cross: (3, 5, 7) - less than one 64-pixel stage, odd H and W (a fixed middle row and column), W % 4 != 0;
(1, 1, 1); (5, 4, 4) - one quad per row; (2, 1, 300) and (2, 300, 1) - degenerate axes (every quad of the second crosses row ends);
(70, 9, 33) - the plane (297) ends inside a stage, row ends walk through the quads, a ragged channel tile; (130, 20, 35) - three channel
tiles (six tile pairs, three of them diagonal), several 256-pixel backward tiles; (64, 16, 64) and (128, 32, 32) - aligned rows, the
16-byte path throughout; (8, 96, 160) - many slabs per tile pair.  Every shape runs all three kinds in one call, with and without row
means, and D is not symmetric."""
import ctypes

import pytest
import torch

import flip_restatement as fr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
KINDS = [fr.LR, fr.UD, fr.ROT180]
NAMES = {fr.LR: "LR", fr.UD: "UD", fr.ROT180: "180"}
SHAPES = [(3, 5, 7), (1, 1, 1), (5, 4, 4), (2, 1, 300), (2, 300, 1), (70, 9, 33), (130, 20, 35), (64, 16, 64), (128, 32, 32), (8, 96, 160)]
CASES = [(shape, cov) for shape in SHAPES for cov in (False, True)]
IDS = [f"{'x'.join(map(str, s))}-{'centred' if c else 'plain'}" for s, c in CASES]


def feature_map(shape):
    g = torch.Generator().manual_seed(23 + sum(shape))
    return torch.relu(torch.randn(*shape, generator=g) + 0.3), g


def scales_of(shape, n):
    C, H, W = shape
    return [1.0 / (C * H * W)] * n


@pytest.fixture(scope="module")
def references():
    """fp64 matrices and gradients per case, computed once."""
    out = {}
    for shape, cov in CASES:
        f, g = feature_map(shape)
        f64 = f.double()
        grams = torch.stack([fr.mirrored_gram(f64, k, cov) for k in KINDS])
        d = torch.randn(len(KINDS), shape[0], shape[0], generator=g)  # not symmetric
        gx = fr.flip_backward(f64, KINDS, [m.double() for m in d], cov)
        base = torch.randn(*shape, generator=g) * float(gx.abs().max())
        out[(shape, cov)] = dict(f=f, grams=grams, d=d, gx=gx, base=base)
    return out


@pytest.mark.parametrize("shape,cov", CASES, ids=IDS)
def test_forward_and_backward_against_fp64(references, shape, cov):
    import hip
    ref = references[(shape, cov)]
    sc = scales_of(shape, len(KINDS))
    f = ref["f"].cuda()
    mean = f.double().mean((1, 2)).float().contiguous() if cov else None
    assert hip.gram_flip_supported(len(KINDS), *shape)
    got = hip.gram_flip_fwd(f, KINDS, sc, mean)
    again = hip.gram_flip_fwd(f, KINDS, sc, mean)
    torch.cuda.synchronize()
    for m, k in enumerate(KINDS):
        e = rel_l2(got[m].cpu(), ref["grams"][m])
        print(f"  G[{NAMES[k]}]: rel-L2 {e:.3e}")
        assert e <= TOL, (NAMES[k], e)
        assert torch.equal(got[m], got[m].t()), NAMES[k]  # bit-symmetric
    assert torch.equal(got, again)  # two calls, equal bits
    dm = ref["d"].cuda()
    gx = torch.full(shape, float("nan"), device="cuda")
    hip.gram_flip_bwd(dm, f, KINDS, sc, mean, gx, False)
    acc = ref["base"].cuda().clone()
    hip.gram_flip_bwd(dm, f, KINDS, sc, mean, acc, True)
    gx2 = torch.empty(shape, device="cuda")
    hip.gram_flip_bwd(dm, f, KINDS, sc, mean, gx2, False)
    torch.cuda.synchronize()
    e0, e1 = rel_l2(gx.cpu(), ref["gx"]), rel_l2(acc.cpu().double() - ref["base"].double(), ref["gx"])
    print(f"  gx: rel-L2 {e0:.3e}, accumulated {e1:.3e}")
    assert e0 <= TOL and e1 <= TOL
    assert torch.equal(gx, gx2)


@pytest.mark.parametrize("shape", [(130, 20, 35), (70, 9, 33)], ids=["130x20x35", "70x9x33"])
def test_each_kind_alone_against_fp64_forward_and_backward(references, shape):
    """One mirror per call: each kind's forward and backward by itself (in the three-mirror calls above a backward error of one kind could
    hide behind the other two), and the bits of a mirror alone are those it has among the three."""
    import hip
    ref = references[(shape, True)]
    f = ref["f"].cuda()
    mean = f.double().mean((1, 2)).float().contiguous()
    sc = scales_of(shape, 1)
    for mu, cov in ((None, False), (mean, True)):
        three = hip.gram_flip_fwd(f, KINDS, scales_of(shape, 3), mu)
        for m, k in enumerate(KINDS):
            alone = hip.gram_flip_fwd(f, [k], sc, mu)
            assert torch.equal(alone[0], three[m]), NAMES[k]
            dm = ref["d"][m:m + 1].cuda().contiguous()
            gx = torch.full(shape, float("nan"), device="cuda")
            hip.gram_flip_bwd(dm, f, [k], sc, mu, gx, False)
            want = fr.flip_backward(ref["f"].double(), [k], [ref["d"][m].double()], cov)
            e = rel_l2(gx.cpu(), want)
            print(f"  {NAMES[k]} alone, {'centred' if cov else 'plain'}: gx rel-L2 {e:.3e}")
            assert e <= TOL, (NAMES[k], e)


def test_a_doubled_kind_gives_two_equal_matrices_and_four_mirrors_run():
    import hip
    shape = (70, 9, 33)
    f = feature_map(shape)[0].cuda()
    kinds = [fr.UD, fr.LR, fr.UD, fr.ROT180]
    got = hip.gram_flip_fwd(f, kinds, scales_of(shape, 4))
    assert torch.equal(got[0], got[2])
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[3])
    three = hip.gram_flip_fwd(f, KINDS, scales_of(shape, 3))
    assert torch.equal(got[1], three[0]) and torch.equal(got[0], three[1]) and torch.equal(got[3], three[2])


def test_a_zero_coef_leaves_its_mirror_out_and_gx_is_still_written():
    import hip
    shape = (70, 9, 33)
    f, g = feature_map(shape)
    d = torch.randn(2, 70, 70, generator=g)
    fc, dc = f.cuda(), d.cuda()
    d_nan = dc.clone()
    d_nan[0] = float("nan")  # never read: its coef is 0
    sc = scales_of(shape, 1)[0]
    gx = torch.full(shape, float("nan"), device="cuda")
    hip.gram_flip_bwd(d_nan, fc, [fr.LR, fr.UD], [0.0, sc], None, gx, False)
    only = torch.empty(shape, device="cuda")
    hip.gram_flip_bwd(dc[1:].contiguous(), fc, [fr.UD], [sc], None, only, False)
    assert torch.equal(gx, only)
    zeros = torch.full(shape, float("nan"), device="cuda")
    hip.gram_flip_bwd(d_nan, fc, [fr.LR, fr.UD], [0.0, 0.0], None, zeros, False)
    assert bool((zeros == 0).all())


def test_mirrors_of_a_degenerate_axis_equal_the_plain_gram():
    """LR on W = 1 and UD on H = 1 are the identity: the matrix is the Gram matrix hip.gram_fwd gives, to the bar of two fp32 sums."""
    import hip
    for shape, kind in (((2, 300, 1), fr.LR), ((2, 1, 300), fr.UD)):
        f = feature_map(shape)[0].cuda()
        got = hip.gram_flip_fwd(f, [kind], scales_of(shape, 1))[0]
        x = f.double().reshape(shape[0], -1).cpu()
        assert rel_l2(got.cpu(), x @ x.t() / f.numel()) <= TOL


def test_a_refused_kind_returns_the_error_and_leaves_the_outputs_unwritten():
    import hip
    C, H, W = 3, 5, 7
    f = feature_map((C, H, W))[0].cuda()
    out = torch.full((2, C, C), 7.0, device="cuda")
    with pytest.raises(hip.HipError, match="kind"):
        hip.gram_flip_fwd(f, [fr.LR, 3], [1.0, 1.0], out=out)
    gx = torch.full((C, H, W), 7.0, device="cuda")
    with pytest.raises(hip.HipError, match="kind"):
        hip.gram_flip_bwd(torch.zeros(2, C, C, device="cuda"), f, [fr.LR, 3], [1.0, 1.0], None, gx, False)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((gx == 7.0).all())
    L = hip.lib()
    one, kinds = (ctypes.c_double * 1)(1.0), (ctypes.c_int * 1)(fr.LR)
    need = L.maua_gram_flip_workspace_bytes(1, C, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out1 = torch.full((1, C, C), 7.0, device="cuda")
    assert L.maua_gram_flip_fwd(f.data_ptr(), None, kinds, one, out1.data_ptr(), 1, C, H, W, ws.data_ptr(), need - 1, None) == -3
    torch.cuda.synchronize()
    assert bool((out1 == 7.0).all())


def test_gram_matrix_module_returns_the_raw_mirrored_product():
    import loss
    shape = (70, 9, 33)
    f, _ = feature_map(shape)
    x = f.cuda()[None].requires_grad_(True)
    g = loss.GramMatrix()
    for kw, kind in ((dict(flip_h=True), fr.LR), (dict(flip_v=True, use_covariance=True), fr.UD), (dict(flip_h=True, flip_v=True), fr.ROT180)):
        cov = bool(kw.get("use_covariance"))
        got = g(x, **kw)
        want = fr.mirrored_gram(f.double(), kind, cov, normalise=False)
        assert got.shape == (70, 70) and rel_l2(got.detach().cpu(), want) <= TOL
        assert torch.equal(got, got.t())
        w = torch.randn(70, 70, generator=torch.Generator().manual_seed(5))
        x.grad = None
        (got * w.cuda()).sum().backward()
        f64 = f.double().requires_grad_(True)
        (fr.mirrored_gram(f64, kind, cov, normalise=False) * w.double()).sum().backward()  # autograd through the means too
        assert rel_l2(x.grad[0].cpu(), f64.grad) <= TOL
