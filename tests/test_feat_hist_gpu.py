"""The feature-histogram kernels (csrc/feat_hist.hip) against the restatement (tests/feat_hist_restatement.py).

Shapes (C, H, W): (3, 5, 7) - less than one vector stage, odd everything; (70, 9, 33) - ragged rows against 16-byte accesses (a plane of 297
elements: every channel but the first starts off a 16-byte boundary); (130, 20, 35); (2, 257, 259) - the launch plan (fh_plan: about 2048
workgroups, chunks of whole 1024-element grains) cuts each channel's 66563 elements into 66 chunks of 1024, the last one 3 elements long,
so one channel's histogram is merged from 66 workgroups and its range from 66 slabs.  (bins, knots) in (16, 2), (256, 1024), (1024, 64).

Inputs: the working map is relu(randn + 0.3), the table the quantiles of relu(2 randn + 1) on a plane of another size, so the residual is
of order 1 and no cancellation; one channel is overwritten with a constant and one with zeros ("degenerate"; with two channels that leaves
no ordinary one, so the split shape also runs without the overwrite).

Bars: lo, hi and every cum entry read back from the state are EQUAL to the restatement's - integers and exact extrema.  loss and gx: rel-L2
2e-5 against fp64, the TOL of tests/test_kernels_gpu.py; a CPU emulation of the fp32 arithmetic of the matching step on these inputs stays
at or below 1.1e-6, which leaves about 20 x for the order of the loss sum.  Both accumulate forms, upstream NULL and a device scalar, and
two runs give the same bits."""
import functools

import numpy as np
import pytest
import torch

import feat_hist_restatement as hr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
CASES = [((3, 5, 7), True), ((70, 9, 33), True), ((130, 20, 35), True), ((2, 257, 259), True), ((2, 257, 259), False)]
PARAMS = [(16, 2), (256, 1024), (1024, 64)]


@functools.lru_cache(maxsize=None)
def inputs(shape, degenerate):
    C, H, W = shape
    gen = torch.Generator().manual_seed(17 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(2 * torch.randn(C, H + 3, W + 5, generator=gen) + 1)
    if degenerate:
        f[C // 2] = 0.625
        f[C - 1] = 0.0
    return f, s


@functools.lru_cache(maxsize=None)
def reference(shape, degenerate, bins, knots):
    """Computed once per case and shared: (table fp32, state, loss, gradient with coef 2 / (C N)) of the restatement."""
    f, s = inputs(shape, degenerate)
    table = hr.quantile_table(s, knots)
    f64, t64 = f.double(), table.double()
    return table, hr.state(f64, bins), float(hr.term(f64, t64, bins)), hr.backward(f64, t64, bins)


def ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else ("degenerate" if v else "plain")


@pytest.mark.parametrize("bins,knots", PARAMS)
@pytest.mark.parametrize("shape,degenerate", CASES, ids=ids)
def test_kernels_against_the_restatement(shape, degenerate, bins, knots):
    import hip
    C, H, W = shape
    N = H * W
    f, s = inputs(shape, degenerate)
    table, (lo_r, hi_r, cum_r), loss_r, grad_r = reference(shape, degenerate, bins, knots)
    assert hip.feat_hist_supported(C, H, W, bins, knots)
    fd, td = f.cuda(), table.cuda()
    assert torch.equal(hip.feat_hist_quantiles(s.cuda(), knots).cpu(), table)  # the capture: sort and gather are exact

    loss, state = hip.feat_hist_fwd(fd, td, bins)
    assert state.numel() * 4 == hip.feat_hist_state_bytes(C, bins)
    lo, hi, cum = (t.cpu() for t in hip.feat_hist_state_parts(state, C, bins))
    assert torch.equal(lo, torch.from_numpy(lo_r)) and torch.equal(hi, torch.from_numpy(hi_r))
    assert torch.equal(cum.long(), torch.from_numpy(cum_r))
    assert bool((cum[:, -1] == N).all()) and bool((cum[:, 0] == 0).all())
    e_loss = abs(float(loss) - loss_r) / abs(loss_r)
    print(f"  loss {float(loss):.9e} (fp64 {loss_r:.9e}): rel {e_loss:.3e}")
    assert loss_r > 1e-2  # (of order 1: not a cancellation)
    assert e_loss <= TOL

    # backward: written (upstream NULL), then accumulated with a device scalar upstream and another coef
    gx = torch.full((C, H, W), float("nan"), device="cuda")
    hip.feat_hist_bwd(fd, td, state, bins, 2.0 / (C * N), gx, False)
    assert bool(torch.isfinite(gx).all())  # every element written
    e_gx = rel_l2(gx.cpu(), grad_r)
    up, coef = -1.75, 0.37
    want_acc = grad_r * (coef * up * C * N / 2.0)
    base = torch.randn(C, H, W, generator=torch.Generator().manual_seed(5)) * float(want_acc.abs().max())
    acc = base.cuda()
    upstream = torch.tensor([up], device="cuda")
    hip.feat_hist_bwd(fd, td, state, bins, coef, acc, True, upstream=upstream)
    e_acc = rel_l2(acc.cpu().double() - base.double(), want_acc)
    print(f"  gx rel-L2 {e_gx:.3e}, accumulated {e_acc:.3e} (bar {TOL:.1e})")
    assert e_gx <= TOL and e_acc <= TOL

    # the same bits again
    loss2, state2 = hip.feat_hist_fwd(fd, td, bins)
    gx2 = torch.empty_like(gx)
    hip.feat_hist_bwd(fd, td, state2, bins, 2.0 / (C * N), gx2, False)
    acc2 = base.cuda()
    hip.feat_hist_bwd(fd, td, state2, bins, coef, acc2, True, upstream=upstream)
    assert torch.equal(state, state2) and torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32)) and torch.equal(acc.view(torch.int32), acc2.view(torch.int32))


def test_planes_that_start_off_a_16_byte_boundary_give_the_same_bits():
    """f, and f and gx differently, one or two elements off a 16-byte boundary: scalar heads of other lengths, and the backward pass without
    quads - the bits of the aligned call."""
    import hip
    shape, bins, knots = (70, 9, 33), 256, 1024
    C, H, W = shape
    f, _ = inputs(shape, True)
    table = reference(shape, True, bins, knots)[0]
    fd, td = f.cuda(), table.cuda()
    loss, state = hip.feat_hist_fwd(fd, td, bins)
    gx = torch.empty_like(fd)
    hip.feat_hist_bwd(fd, td, state, bins, 1.0, gx, False)
    for off_f, off_g in ((1, 1), (2, 0), (3, 1), (0, 3)):
        buf = torch.zeros(f.numel() + 8, device="cuda")
        fo = buf[off_f:off_f + f.numel()].view(C, H, W)
        fo.copy_(fd)
        assert fo.data_ptr() % 16 == 4 * off_f and fo.is_contiguous()
        loss_o, state_o = hip.feat_hist_fwd(fo, td, bins)
        assert torch.equal(state_o, state) and torch.equal(loss_o.view(torch.int32), loss.view(torch.int32)), (off_f, off_g)
        gbuf = torch.full((f.numel() + 8,), 7.0, device="cuda")
        go = gbuf[off_g:off_g + f.numel()].view(C, H, W)
        hip.feat_hist_bwd(fo, td, state_o, bins, 1.0, go, False)
        assert torch.equal(go.view(torch.int32), gx.view(torch.int32)), (off_f, off_g)
        assert bool((gbuf[:off_g] == 7.0).all()) and bool((gbuf[off_g + f.numel():] == 7.0).all())  # nothing beside gx written


def test_autograd_function_and_module_errors():
    """loss._FeatHistFn: forward = the kernel's loss, backward = the kernel's gradient times the incoming one; a module in loss mode without
    a captured table raises."""
    import hip
    import loss as loss_mod
    shape, bins, knots = (70, 9, 33), 256, 1024
    C, H, W = shape
    f, _ = inputs(shape, True)
    table, _, loss_r, grad_r = reference(shape, True, bins, knots)
    x = f.cuda().unsqueeze(0).requires_grad_(True)
    h = loss_mod._FeatHistFn.apply(x, table.cuda(), bins)
    (3.0 * h).backward()
    assert abs(float(h.detach()) - loss_r) <= TOL * loss_r and rel_l2(x.grad[0].cpu(), 3.0 * grad_r) <= TOL
    m = loss_mod.StyleLoss(1.0)
    m.name = "style_hist"
    m.hist_loss_factor = 1.0
    m.mode, m.blend_weight = "loss", 1.0
    m.target = torch.zeros(C, C, device="cuda")
    with pytest.raises(RuntimeError, match="feature-histogram target not captured"):
        m(x.detach())
    with pytest.raises(hip.HipError, match="not supported"):
        hip.feat_hist_fwd(f.cuda(), table.cuda(), 8)
