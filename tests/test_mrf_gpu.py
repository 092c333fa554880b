"""The MRF patch-matching kernels (csrc/mrf.hip) against the restatement (tests/mrf_restatement.py).

Shapes (C, H, W, Hs, Ws, stride) - a workgroup of the match owns 256 queries and walks its slice of the bank in tiles of 128 patches,
16 channels per stage:
    (2, 3, 3, 3, 3, 1)        Q = P = 1
    (3, 5, 7, 6, 9, 1)        Q = 15, P = 28: everything inside one tile
    (70, 9, 33, 12, 31, 1)    Q = 217, P = 290: a channel tail (70 = 4 x 16 + 6), three style tiles, each a slice of its own
    (130, 20, 35, 23, 40, 2)  Q = 594 in three query tiles, a strided bank of P = 209 in two tiles, nine channel blocks
    (16, 66, 70, 67, 131, 1)  Q = 4352 in 17 query tiles, P = 8385 in 66 style tiles: 33 slices of 2 tiles, so the merge has work to do
Inputs: relu(randn + 0.3), seeded.

Bars.  Decisions: for every query the fp64 score of the chosen patch is at least (1 - 2e-5) times the best fp64 score (2e-5 = TOL of
tests/test_kernels_gpu.py), and nn[q] EQUALS the restatement's wherever the fp64 relative margin between the best and the second-best score
exceeds 2e-5; at most 1 % of the queries may lie below that margin (asserted; on these inputs the restatement finds at most 0.12 %).  With
nn read back and pinned in the restatement: loss and gx within rel 2e-5 of fp64.  inv: one fp32 ulp (the fp64 sum in another order,
rounded once).  Planted answers, ties and repeated calls: exact."""
import functools

import pytest
import torch

import mrf_restatement as mr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = [(2, 3, 3, 3, 3, 1), (3, 5, 7, 6, 9, 1), (70, 9, 33, 12, 31, 1), (130, 20, 35, 23, 40, 2), (16, 66, 70, 67, 131, 1)]


def ids(v):
    return "x".join(str(i) for i in v)


@functools.lru_cache(maxsize=None)
def inputs(shape):
    C, H, W, Hs, Ws, stride = shape
    gen = torch.Generator().manual_seed(23 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(torch.randn(C, Hs, Ws, generator=gen) + 0.3)
    s_map, origin, inv, used = mr.build_bank([s], stride, 1 << 20)
    assert used == stride and origin.numel() == len(range(0, Hs - 2, stride)) * len(range(0, Ws - 2, stride))
    return f, s_map, origin, inv


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Computed once per shape and shared: (fp64 scores (Q, P), nn of the restatement, best score, relative margin)."""
    f, s, origin, inv = inputs(shape)
    sc = mr.scores(f, s, origin, inv)
    best, margin = mr.margins(sc)
    return sc, mr.nearest(sc), best, margin


def run(f, s, origin):
    import hip
    fd, sd = f.cuda(), s.cuda()
    od, inv = hip.mrf_bank(sd, origin)
    loss, state = hip.mrf_fwd(fd, sd, od, inv)
    return fd, sd, od, inv, loss, state


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_against_the_restatement(shape):
    import hip
    C, H, W, Hs, Ws, stride = shape
    Q = (H - 2) * (W - 2)
    f, s, origin, inv_r = inputs(shape)
    sc, nn_r, best_r, margin = reference(shape)
    P = origin.numel()
    assert hip.mrf_supported(C, H, W, Hs, Ws, P)
    fd, sd, od, inv, loss, state = run(f, s, origin)
    assert state.numel() * 4 == hip.mrf_state_bytes(H, W) == 8 * Q
    e_inv = float(((inv.cpu().double() - inv_r.double()).abs() / inv_r.double()).max())
    print(f"  inv: rel {e_inv:.3e} (one fp32 ulp: 1.2e-7)")
    assert e_inv <= 2.0 ** -23

    nn, best = (t.cpu() for t in hip.mrf_state_parts(state, H, W))
    assert int(nn.min()) >= 0 and int(nn.max()) < P
    # 1. the score of the chosen patch
    chosen = sc[torch.arange(Q), nn.long()]
    short = float(((best_r - chosen) / best_r).max())
    print(f"  Q {Q}, P {P}: chosen score short of the best by at most {short:.3e} (bar {TOL:.1e})")
    assert bool((chosen >= (1 - TOL) * best_r).all())
    assert rel_l2(best, best_r) <= TOL
    # 2. the same patch wherever the margin is clear
    clear = margin > TOL
    share = 1.0 - float(clear.double().mean())
    differ = int((nn.long() != nn_r).sum())
    print(f"  {share * 100:.3f} % of the queries below the margin; {differ} decisions differ from fp64")
    assert share <= 0.01
    assert torch.equal(nn.long()[clear], nn_r[clear])

    # 5. loss and gradient with the device's decisions pinned
    loss_r = float(mr.loss(f, s, origin, nn))
    e_loss = abs(float(loss) - loss_r) / abs(loss_r)
    print(f"  loss {float(loss):.9e} (fp64 {loss_r:.9e}): rel {e_loss:.3e}")
    assert loss_r > 1e-2 and e_loss <= TOL
    grad_r = mr.gather_gradient(f, s, origin, nn)
    gx = torch.full((C, H, W), float("nan"), device="cuda")
    hip.mrf_bwd(fd, sd, od, state, 2.0 / (9 * C * Q), gx, False)
    assert bool(torch.isfinite(gx).all())  # every element written
    e_gx = rel_l2(gx.cpu(), grad_r)
    up, coef = -1.75, 0.37
    want_acc = mr.gather_gradient(f, s, origin, nn, coef=coef * up)
    base = torch.randn(C, H, W, generator=torch.Generator().manual_seed(5)) * float(want_acc.abs().max())
    acc = base.cuda()
    upstream = torch.tensor([up], device="cuda")
    hip.mrf_bwd(fd, sd, od, state, coef, acc, True, upstream=upstream)
    e_acc = rel_l2(acc.cpu().double() - base.double(), want_acc)
    print(f"  gx rel-L2 {e_gx:.3e}, accumulated {e_acc:.3e} (bar {TOL:.1e})")
    assert e_gx <= TOL and e_acc <= TOL

    # 6. the same bits again
    _, _, od2, inv2, loss2, state2 = run(f, s, origin)
    gx2 = torch.empty_like(gx)
    hip.mrf_bwd(fd, sd, od2, state2, 2.0 / (9 * C * Q), gx2, False)
    acc2 = base.cuda()
    hip.mrf_bwd(fd, sd, od2, state2, coef, acc2, True, upstream=upstream)
    assert torch.equal(inv.view(torch.int32), inv2.view(torch.int32))
    assert torch.equal(state, state2) and torch.equal(loss.view(torch.int32), loss2.view(torch.int32))
    assert torch.equal(gx.view(torch.int32), gx2.view(torch.int32)) and torch.equal(acc.view(torch.int32), acc2.view(torch.int32))


@pytest.mark.parametrize("dims", [(3, 5, 7, 6, 10), (16, 20, 30, 40, 64)], ids=ids)
def test_equal_patches_go_to_the_lowest_index(dims):
    """3. A style map whose right half repeats its left half bit for bit: every patch inside the left half has a twin of higher index, some
    in the same style tile, some in a later slice ((16, 20, 30, 40, 64): P = 2356 in 19 slices, two query tiles).  nn[q] is never a patch
    that has an identical patch of lower index - a merge that took the slices out of order, or a comparison that let an equal score win,
    would name the twin."""
    import hip
    C, H, W, Hs, Ws = dims
    gen = torch.Generator().manual_seed(31 + C)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    left = torch.relu(torch.randn(C, Hs, Ws // 2, generator=gen) + 0.3)
    s_map, origin, inv_r, _ = mr.build_bank([torch.cat([left, left], dim=2)], 1, 1 << 20)
    rows = mr.bank_patches(s_map, origin)
    first, seen = [], {}
    for p in range(rows.shape[0]):
        first.append(seen.setdefault(rows[p].numpy().tobytes(), p))
    first = torch.tensor(first)
    twins = int((first != torch.arange(rows.shape[0])).sum())
    assert twins == (Hs - 2) * (Ws // 2 - 2)
    _, _, _, inv, _, state = run(f, s_map, origin)
    assert torch.equal(inv.cpu()[first], inv.cpu())  # equal patches, equal norms: the scores of twins are bit-equal
    nn = hip.mrf_state_parts(state, H, W)[0].cpu().long()
    named = int((first[nn] != nn).sum())
    print(f"  {twins} of {rows.shape[0]} patches have a twin of lower index; {named} of {nn.numel()} queries name one")
    assert named == 0  # (the restatement is not asked: a BLAS matmul need not give equal columns equal bits)
    # and the winners are patches whose twin scores the same: the test would notice
    assert int((first == nn[:, None]).sum(1).max()) == 2


@pytest.mark.parametrize("dims", [(3, 6, 9, 5, 7, 1, 2), (16, 67, 131, 20, 35, 30, 60)], ids=ids)
def test_a_window_cut_out_of_the_style_map_finds_its_origin(dims):
    """4. F is a window of S, stride 1: nn[q] is the origin it was cut from wherever the restatement finds no equal-scoring patch, the loss
    is exactly 0, gx exactly 0 when written and bit-unchanged when accumulated into."""
    import hip
    C, Hs, Ws, H, W, y0, x0 = dims
    gen = torch.Generator().manual_seed(37 + C)
    s = torch.relu(torch.randn(C, Hs, Ws, generator=gen) + 0.3)
    s_map, origin, inv_r, _ = mr.build_bank([s], 1, 1 << 20)
    assert origin.numel() == (Hs - 2) * (Ws - 2)  # (no patch of norm 0: origin[p] = p's place on the full grid)
    f = s[:, y0:y0 + H, x0:x0 + W].contiguous()
    sc = mr.scores(f, s_map, origin, inv_r)
    alone = (sc == sc.max(dim=1, keepdim=True).values).sum(1) == 1
    planted = torch.tensor([(y0 + y) * Ws + x0 + x for y in range(H - 2) for x in range(W - 2)])
    assert torch.equal(origin.long()[mr.nearest(sc)][alone], planted[alone]) and bool(alone.all())
    fd, sd, od, inv, loss, state = run(f, s_map, origin)
    nn = hip.mrf_state_parts(state, H, W)[0].cpu().long()
    assert torch.equal(origin.long()[nn][alone], planted[alone])
    assert float(loss) == 0.0
    gx = torch.full((C, H, W), float("nan"), device="cuda")
    hip.mrf_bwd(fd, sd, od, state, 0.37, gx, False, upstream=torch.tensor([-1.75], device="cuda"))
    assert bool((gx == 0).all())
    base = torch.randn(C, H, W, generator=gen)
    acc = base.cuda()
    hip.mrf_bwd(fd, sd, od, state, 0.37, acc, True, upstream=torch.tensor([-1.75], device="cuda"))
    assert torch.equal(acc.cpu().view(torch.int32), base.view(torch.int32))


def test_refusals_come_before_any_launch():
    """7. maua_mrf_supported and the three error codes, with device pointers: nothing the calls were handed changes."""
    import hip
    L = hip.lib()
    shape = SHAPES[1]
    C, H, W, Hs, Ws, _ = shape
    f, s, origin, _ = inputs(shape)
    P = origin.numel()
    fd, sd, od, inv, loss, state = run(f, s, origin)
    torch.cuda.synchronize()
    keep = (state.clone(), loss.clone(), inv.clone())
    ws = torch.full((hip.mrf_workspace_bytes(C, H, W, Hs, Ws, P),), 0x5A, dtype=torch.uint8, device="cuda")
    gx = torch.full((C, H, W), 7.0, device="cuda")
    ptr = lambda t: t.data_ptr()  # noqa: E731
    fwd = lambda c, h, w, hs, wsz, p, wbytes, f_=fd: L.maua_mrf_fwd(  # noqa: E731
        ptr(f_) if f_ is not None else None, ptr(sd), ptr(od), ptr(inv), ptr(state), ptr(loss), c, h, w, hs, wsz, p, ptr(ws), wbytes, hip._stream())
    bwd = lambda c, h, w, hs, wsz, p, gx_=gx: L.maua_mrf_bwd(  # noqa: E731
        ptr(fd), ptr(sd), ptr(od), ptr(state), None, 1.0, ptr(gx_) if gx_ is not None else None, c, h, w, hs, wsz, p, 0, hip._stream())
    assert L.maua_mrf_supported(C, H, W, Hs, Ws, P) == 1
    for bad in ((0, H, W, Hs, Ws, P), (1025, H, W, Hs, Ws, P), (C, 2, W, Hs, Ws, P), (C, H, 2, Hs, Ws, P), (C, H, W, 2, Ws, P), (C, H, W, Hs, 2, P),
                (C, 1 << 15, 1 << 15, Hs, Ws, P), (C, H, W, Hs, Ws, 0), (C, H, W, Hs, Ws, (1 << 20) + 1)):
        assert L.maua_mrf_supported(*bad) == 0 and L.maua_mrf_workspace_bytes(*bad) == 0, bad
        assert fwd(*bad, ws.numel()) == -2 and bwd(*bad) == -2, bad  # MAUA_E_UNSUPPORTED
    for bad in ((0, Hs, Ws, P), (1025, Hs, Ws, P), (C, 2, Ws, P), (C, Hs, 2, P), (C, 1 << 15, 1 << 15, P), (C, Hs, Ws, 0), (C, Hs, Ws, (1 << 20) + 1)):
        assert L.maua_mrf_bank(ptr(sd), ptr(od), ptr(inv), *bad, hip._stream()) == -2, bad
    assert fwd(C, H, W, Hs, Ws, P, ws.numel(), f_=None) == -1 and bwd(C, H, W, Hs, Ws, P, gx_=None) == -1  # MAUA_E_INVAL
    assert L.maua_mrf_bank(None, ptr(od), ptr(inv), C, Hs, Ws, P, hip._stream()) == -1
    assert fwd(C, H, W, Hs, Ws, P, ws.numel() - 1) == -3 and fwd(C, H, W, Hs, Ws, P, 0) == -3  # MAUA_E_WORKSPACE
    with pytest.raises(hip.HipError, match="leaves the"):
        hip.mrf_bank(sd, torch.tensor([0, (Hs - 2) * Ws], dtype=torch.int32))
    with pytest.raises(hip.HipError, match="leaves the"):
        hip.mrf_bank(sd, torch.tensor([Ws - 2], dtype=torch.int32))
    with pytest.raises(hip.HipError, match="host int32"):
        hip.mrf_bank(sd, od)
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((gx == 7.0).all())
    assert torch.equal(state, keep[0]) and torch.equal(loss, keep[1]) and torch.equal(inv, keep[2])


def test_autograd_function_and_module_errors():
    """loss._MrfFn: forward = the kernel's loss, backward = the kernel's gradient times the incoming one; a module in loss mode without a
    captured bank raises; a module that captured two maps builds the restatement's bank."""
    import loss as loss_mod
    shape = SHAPES[2]
    C, H, W, Hs, Ws, _ = shape
    f, s, origin, _ = inputs(shape)
    fd, sd, od, inv, loss, state = run(f, s, origin)
    import hip
    nn = hip.mrf_state_parts(state, H, W)[0].cpu()
    x = fd.unsqueeze(0).requires_grad_(True)
    m = loss_mod._MrfFn.apply(x, sd, od, inv)
    (3.0 * m).backward()
    assert torch.equal(m.detach().reshape(1), loss)
    assert rel_l2(x.grad[0].cpu(), 3.0 * mr.gather_gradient(f, s, origin, nn)) <= TOL
    mod = loss_mod.StyleLoss(1.0)
    mod.name = "style_mrf"
    mod.mrf_factor = 1.0
    mod.mode, mod.blend_weight = "loss", 1.0
    mod.target = torch.zeros(C, C, device="cuda")
    with pytest.raises(RuntimeError, match="MRF patch bank not captured"):
        mod(x.detach())
    # capture: two maps of different widths, one with a block of zeros, stride and cap as the restatement has them
    gen = torch.Generator().manual_seed(3)
    a, b = torch.relu(torch.randn(C, 9, 14, generator=gen) + 0.3), torch.relu(torch.randn(C, 12, 8, generator=gen) + 0.3)
    a[:, :5, :6] = 0.0
    mod.mode, mod.mrf_stride, mod.mrf_max_patches = "capture", 1, 100
    mod.reset_targets()
    for t in (a, b):
        mod(t.cuda().unsqueeze(0))
    mod.mode = "loss"
    mod(x.detach())
    s_r, origin_r, inv_r, used = mr.build_bank([a, b], 1, 100)
    assert used == 2 and origin_r.numel() < len(mr.grid([(9, 14), (12, 8)], 1, 100)[1])  # the cap raised the stride; zero patches left out
    assert torch.equal(mod.mrf_bank[0].cpu(), s_r) and torch.equal(mod.mrf_bank[1].cpu(), origin_r)
    assert float(((mod.mrf_bank[2].cpu().double() - inv_r.double()).abs() / inv_r.double()).max()) <= 2.0 ** -23
    mod.reset_targets()
    assert mod.mrf_bank is None and mod._mrf_maps == []
