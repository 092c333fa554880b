"""The sliced Wasserstein kernels (csrc/swd.hip) against the restatement (tests/swd_restatement.py).

Shapes (C, D, H, W): (3, 5, 5, 7) - less than one tile in every dimension, odd everything; (70, 70, 9, 33) - ragged C and D against the 16-
and 32-wide blocks, rows of 297 elements off 16-byte boundaries; (130, 64, 20, 35) - D < C: the projection's K runs over eight stages of 16
channels and a ninth of 2, the backward's rows over one block of 128 channels and one of 2; (64, 96, 16, 16) - D > C, everything aligned; (2, 2, 257, 259) - rows of 66563 elements cut into 261 pixel tiles, the
last one partial, a direction's range folded from 261 slabs and its histogram merged from 66 workgroups.  (bins, knots) in (16, 2),
(256, 1024), (1024, 64).

Inputs: the working map is relu(randn + 0.3), the style map relu(2 randn + 1) on (H + 3, W + 5), the directions those of the restatement; for
D > 2 one row of V is set to zero - a constant projection, which takes the hi == lo path.

Bars: the projection read back after maua_swd_project is within 2e-5 (rel-L2; TOL of tests/test_kernels_gpu.py, about 100 x the distance of
an fp32 projection from fp64 on these inputs) of fp64 V F.  Everything behind it is compared on the read-back P: lo, hi and every cum entry
of the state EQUAL to the restatement's and to the state hip.feat_hist_fwd leaves for the same P (which holds the fused range epilogue and
the counter zeroing to the unfused path), the loss within 2e-5 (asserted > 1e-2: nothing cancels), G = P - R as left in P's buffer and the
backward in both accumulate forms within 2e-5.  Two runs give the same bits, and the plain projection (state NULL) the same P."""
import functools

import pytest
import torch

import feat_hist_restatement as hr
import swd_restatement as wr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = [(3, 5, 5, 7), (70, 70, 9, 33), (130, 64, 20, 35), (64, 96, 16, 16), (2, 2, 257, 259)]
PARAMS = [(16, 2), (256, 1024), (1024, 64)]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(f, directions, style map, fp64 projection of f), computed once per shape and shared."""
    C, D, H, W = shape
    gen = torch.Generator().manual_seed(19 + C + D + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(2 * torch.randn(C, H + 3, W + 5, generator=gen) + 1)
    v = wr.directions(C, D, 0, 0).clone()
    if D > 2:
        v[D // 2] = 0.0
    return f, v, s, wr.project(f, v)


@functools.lru_cache(maxsize=None)
def table_of(shape, knots):
    f, v, s, _ = inputs(shape)
    return wr.table(s, v, knots).float()


def ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def run(fd, vd, vtd, td, bins, base, up, coef):
    """One forward and both backward forms -> (P, state, loss, G, gx, accumulated gx), device tensors."""
    import hip
    C, D = vtd.shape
    H, W = fd.shape[-2:]
    proj, state, ws = hip.swd_project(fd, vd, bins)
    p = proj.clone()
    loss = hip.swd_match(proj, td, state, bins, ws)
    gx = torch.full((C, H, W), float("nan"), device="cuda")
    hip.swd_bwd(proj, vtd, 2.0 / (D * H * W), gx, False)
    acc = base.cuda()
    hip.swd_bwd(proj, vtd, coef, acc, True, upstream=torch.tensor([up], device="cuda"))
    return p, state, loss, proj, gx, acc


@pytest.mark.parametrize("bins,knots", PARAMS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_against_the_restatement(shape, bins, knots):
    import hip
    C, D, H, W = shape
    N = H * W
    f, v, s, p64 = inputs(shape)
    table = table_of(shape, knots)
    t64 = table.double()
    assert hip.swd_supported(C, D, H, W, bins, knots)
    fd, vd, vtd, td = f.cuda(), v.cuda(), v.t().contiguous().cuda(), table.cuda()
    up, coef = -1.75, 0.37
    scale = float((2.0 / (D * N)) * p64.abs().max())
    base = torch.randn(C, H, W, generator=torch.Generator().manual_seed(5)) * scale
    pd, state, loss, gd, gx, acc = run(fd, vd, vtd, td, bins, base, up, coef)
    torch.cuda.synchronize()

    # projection
    p = pd.cpu()
    e_p = rel_l2(p, p64)
    print(f"  projection rel-L2 {e_p:.3e} (bar {TOL:.1e})")
    assert e_p <= TOL
    if D > 2:
        assert bool((p[D // 2] == 0).all())
    # state, on the read-back P
    assert state.numel() * 4 == hip.swd_state_bytes(D, bins)
    lo_r, hi_r, cum_r = hr.state(p, bins)
    lo, hi, cum = (t.cpu() for t in hip.feat_hist_state_parts(state, D, bins))
    assert torch.equal(lo, torch.from_numpy(lo_r)) and torch.equal(hi, torch.from_numpy(hi_r))
    assert torch.equal(cum.long(), torch.from_numpy(cum_r))
    assert bool((cum[:, -1] == N).all()) and bool((cum[:, 0] == 0).all())
    # cross-check: the unfused path on the same P
    loss_fh, state_fh = hip.feat_hist_fwd(pd, td, bins)
    assert torch.equal(state_fh, state)
    assert abs(float(loss_fh) - float(loss)) <= TOL * float(loss)
    # loss
    loss_r = float(hr.term(p.double(), t64, bins))
    e_loss = abs(float(loss) - loss_r) / abs(loss_r)
    print(f"  loss {float(loss):.9e} (fp64 {loss_r:.9e}): rel {e_loss:.3e}")
    assert loss_r > 1e-2  # (of order 1: not a cancellation)
    assert e_loss <= TOL
    # G, as left in P's buffer
    g_r = wr.residual(p, t64, bins)
    e_g = rel_l2(gd.cpu(), g_r)
    # backward: written into NaNs with upstream NULL, accumulated onto a random base with a device scalar
    assert bool(torch.isfinite(gx).all())  # every element written
    e_gx = rel_l2(gx.cpu(), wr.backward(p, v, t64, bins))
    want_acc = wr.backward(p, v, t64, bins, coef=coef, upstream=up)
    e_acc = rel_l2(acc.cpu().double() - base.double(), want_acc)
    print(f"  G rel-L2 {e_g:.3e}, gx {e_gx:.3e}, accumulated {e_acc:.3e} (bar {TOL:.1e})")
    assert e_g <= TOL and e_gx <= TOL and e_acc <= TOL

    # the same bits again, and the plain projection
    again = run(fd, vd, vtd, td, bins, base, up, coef)
    for a, b in zip((pd, state, loss, gd, gx, acc), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    plain, none_state, none_ws = hip.swd_project(fd, vd)
    assert none_state is None and none_ws is None and torch.equal(plain.view(torch.int32), pd.view(torch.int32))


@pytest.mark.parametrize("bins,knots", PARAMS, ids=ids)
def test_identity_directions_give_the_feature_histogram_entry_points(bins, knots):
    import hip
    C, D, H, W = 70, 70, 9, 33
    f, _, s, _ = inputs((C, D, H, W))
    table = hr.quantile_table(s, knots)
    fd, td, eye = f.cuda(), table.cuda(), torch.eye(C).cuda()
    proj, state, ws = hip.swd_project(fd, eye, bins)
    assert torch.equal(proj, fd)  # (one product by 1 and zeros)
    loss = hip.swd_match(proj, td, state, bins, ws)
    gx = torch.empty_like(fd)
    hip.swd_bwd(proj, eye, 2.0 / (C * H * W), gx, False)
    loss_fh, state_fh = hip.feat_hist_fwd(fd, td, bins)
    gx_fh = torch.empty_like(fd)
    hip.feat_hist_bwd(fd, td, state_fh, bins, 2.0 / (C * H * W), gx_fh, False)
    assert torch.equal(state, state_fh)
    assert abs(float(loss) - float(loss_fh)) <= TOL * float(loss_fh) and float(loss_fh) > 1e-2
    assert rel_l2(gx.cpu(), gx_fh.cpu()) <= TOL


def test_autograd_function_and_module():
    """loss._SwdFn: forward = the kernels' loss, backward = the kernels' gradient times the incoming one, through hip.swd_project and
    hip.swd_match as the module attributes name them; a module captures its table from the plain projection and raises without it."""
    import hip
    import loss as loss_mod
    shape, bins, knots = (70, 70, 9, 33), 256, 1024
    C, D, H, W = shape
    f, v, s, _ = inputs(shape)
    table = table_of(shape, knots)
    seen = []
    real = hip.swd_project

    def recording(*a, **k):
        out = real(*a, **k)
        seen.append(out[0].clone())
        return out

    hip.swd_project = recording
    try:
        x = f.cuda().unsqueeze(0).requires_grad_(True)
        val = loss_mod._SwdFn.apply(x, v.cuda(), v.t().contiguous().cuda(), table.cuda(), bins)
        (3.0 * val).backward()
    finally:
        hip.swd_project = real
    assert len(seen) == 1
    p = seen[0].cpu()
    want = float(hr.term(p.double(), table.double(), bins))
    assert abs(float(val.detach()) - want) <= TOL * want
    assert rel_l2(x.grad[0].cpu(), 3.0 * wr.backward(p, v, table.double(), bins)) <= TOL

    m = loss_mod.StyleLoss(1.0)
    m.name = "style_swd"
    m.swd_factor, m.swd_directions, m.swd_knots, m.swd_index, m.swd_seed = 1.0, 16, 64, 2, 5
    m.mode, m.blend_weight = "loss", 1.0
    m.target = torch.zeros(C, C, device="cuda")
    with pytest.raises(RuntimeError, match="sliced Wasserstein target not captured"):
        m(x.detach())
    m.reset_targets()
    m.mode = "capture"
    m(s.cuda().unsqueeze(0))
    dirs = wr.directions(C, 16, 5, 2)
    assert torch.equal(m._swd_dirs[0].cpu(), dirs) and torch.equal(m._swd_dirs[1].cpu(), dirs.t())
    assert tuple(m.swd_target.shape) == (16, 64)
    assert rel_l2(m.swd_target.cpu(), wr.table(s, dirs, 64)) <= TOL
    with pytest.raises(hip.HipError, match="not supported"):
        hip.swd_project(f.cuda(), v.cuda(), 8)
