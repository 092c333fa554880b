"""The guided layer's fused finish and masked backward (csrc/gram_guided.hip: maua_guided_gram_fwd_mse_ledger, maua_guided_gram_bwd_masked)
against the plain guided kernels (bit for bit) and fp64.

Shapes: those of tests/test_containment_guided_gpu.py - channels that are no multiple of the 64-channel tile (one ragged tile pair, three
pairs), planes that end inside a 64-pixel stage and inside the backward kernel's 256-pixel tile, one plane smaller than a stage - and two
with eight regions of 450 and 650 channels on a short plane, where the finishing launch has to take fewer workgroups per tile pair.
Regions: hard, soft, massless (scale 0), a soft one whose grad_scale and loss_scale are 0, further soft ones.  Bars: D against fp64 at
2e-5 rel-L2 (the contraction bar of tests/test_gram_guided_gpu.py; D is a difference of two matrices, so the targets lie about a matrix
norm away from the Gram matrices and the bar is relative to a quantity of the operands' size), the loss at 1e-5 relative (the per-slot
loss bar of tests/test_guided_style_gpu.py)."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
TOL_LOSS = 1e-5
# (C, N, covariance form, regions); the last two: eight regions of so many channels that the finishing launch takes 8, then 4 workgroups per
# tile pair instead of 16 (8 x 36 x 16 and 8 x 66 x 8 partial sums would not fit one ledger record)
SHAPES = [(70, 297, True, 4), (70, 297, False, 4), (3, 5, True, 4), (130, 700, True, 4), (450, 70, False, 8), (650, 70, True, 8)]


def inputs(C, N, R):
    gen = torch.Generator().manual_seed(77 + C + N)
    f = torch.relu(torch.randn(C, N, generator=gen) + 0.3)
    g = torch.rand(R, N, generator=gen)     # (regions 4 and up: soft)
    g[:4] = 0
    g[0, N // 3:] = 1                       # hard: zero over the first third
    g[1] = torch.rand(N, generator=gen)     # soft
    g[2, 0] = 0.5                           # mass 0.25: inactive (scale 0)
    g[3] = torch.rand(N, generator=gen)     # soft, but given grad_scale = loss_scale = 0
    return f, g, gen


def reference(f, g, cov):
    f64, g64 = f.double(), g.double()
    C = f.shape[0]
    mass = (g64 * g64).sum(1)
    grams, means, scale = [], [], []
    for r in range(g.shape[0]):
        act = bool(mass[r] >= 1.0)
        mu = (f64 * (g64[r] ** 2)[None]).sum(1) / mass[r] if (cov and act) else torch.zeros(C, dtype=torch.float64)
        x = (f64 - mu[:, None]) * g64[r][None]
        scale.append(1.0 / (C * float(mass[r])) if act else 0.0)
        grams.append(x @ x.t() * scale[-1])
        means.append(mu)
    return torch.stack(grams), torch.stack(means), mass, torch.tensor(scale, dtype=torch.float64)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"C{p[0]}-N{p[1]}-{'cov' if p[2] else 'gram'}-R{p[3]}")
def case(request):
    C, N, cov, R = request.param
    f, g, gen = inputs(C, N, R)
    g64, mean64, mass64, scale64 = reference(f, g, cov)
    t = torch.randn(R, C, C, generator=gen, dtype=torch.float64)
    # symmetric targets a matrix norm away from the Gram matrices (a captured target is a Gram matrix: symmetric)
    target64 = g64 + (t + t.transpose(1, 2)) * (g64.norm() / 4 / (C + 1))
    return dict(C=C, N=N, cov=cov, f=f.cuda(), g=g.cuda(), gen=gen, g64=g64, mean64=mean64, mass=mass64.cuda(), scale=scale64.float().cuda(),
                scale64=scale64, target=target64.float().cuda())


def test_fused_forward_against_the_plain_forward_and_fp64(case):
    import hip
    C, N, cov, f, g, scale, mass, target = (case[k] for k in ("C", "N", "cov", "f", "g", "scale", "mass", "target"))
    R = g.shape[0]
    assert hip.gram_guided_mse_ledger_supported(R, C)
    ls = torch.tensor([0.5 / (C * C), 0.25 / (C * C), 0.125 / (C * C), 0.0] + [0.3 / (C * C)] * (R - 4)).cuda()
    gs = torch.tensor([3.0 / (C * C), 1.5 / (C * C), 2.0 / (C * C), 0.0] + [1.1 / (C * C)] * (R - 4)).cuda()
    plain, plain_mean = hip.gram_guided_fwd(f, g, scale, cov, mass)
    slots, slot = 3, 1
    runs = []
    for _ in range(2):
        led = hip.loss_ledger(1, slots, f.device)
        gram = torch.full((R, C, C), float("nan"), device="cuda")
        dmat = torch.full((R, C, C), float("nan"), device="cuda")
        mean = torch.full((R, C), float("nan"), device="cuda") if cov else None
        hip.gram_guided_fwd_mse_ledger(f, g, scale, cov, mass, gram, mean, target, dmat, ls, gs, led[0], slot)
        record = led[0, slot].clone()
        losses, total = torch.zeros(1, slots, device="cuda"), torch.zeros(1, device="cuda")
        exact = torch.zeros(1, slots, dtype=torch.float64, device="cuda")
        hip.loss_ledger_sum(led, losses, total, exact)
        torch.cuda.synchronize()
        runs.append((gram, dmat, mean, record, losses, exact))
    (gram, dmat, mean, record, losses, exact), second = runs
    for a, b in zip(runs[0], second):
        assert (a is None and b is None) or torch.equal(a, b), "two runs differ"
    assert torch.equal(gram, plain), "gram: not the bits of gram_guided_fwd"
    assert (mean is None and plain_mean is None) or torch.equal(mean, plain_mean)
    pairs = ((C + 63) // 64) * ((C + 63) // 64 + 1) // 2
    assert float(record[1]) == 1.0 and int(record[0]) == max(q for q in (4, 8, 16) if R * pairs * q <= 4096) * R * pairs
    assert not bool(led[0, [0, 2]].any()), "a neighbouring record was written"
    t64, g64 = target.double().cpu(), case["g64"]
    for r in range(R):
        assert torch.equal(dmat[r], dmat[r].t()), f"D of region {r} is not exactly symmetric"
    scale64 = case["scale64"]
    assert scale64[2] == 0 and not bool(gram[2].any()) and not bool(dmat[2].any()), "massless region"
    assert not bool(dmat[3].any()), "region with grad_scale = 0"
    assert scale64[0] != 0
    for r in [0, 1] + list(range(4, R)):
        if scale64[r] == 0:  # (the soft guide over the five-pixel plane can have a mass below 1: inactive, exact zeros)
            assert not bool(gram[r].any()) and not bool(dmat[r].any())
            continue
        want = float(gs[r].double()) * (g64[r] - t64[r])
        e = rel_l2(dmat[r].cpu(), want)
        print(f"  D[{r}] rel-L2 {e:.3e}")
        assert e <= TOL, (r, e)
    # the massless region's matrix is zeros: its loss term is loss_scale x sum T^2
    want = sum(float(ls[r].double()) * float(((g64[r] if r != 2 else 0 * g64[r]) - t64[r]).pow(2).sum()) for r in range(R))
    got = float(exact[0, slot])
    print(f"  loss {got:.9e} (fp64 {want:.9e}), fp32 slot {float(losses[0, slot]):.9e}")
    assert abs(got - want) <= TOL_LOSS * abs(want)
    assert abs(float(losses[0, slot]) - want) <= TOL_LOSS * abs(want)
    assert float(total[0]) == float(losses[0, slot])


def test_masked_backward(case):
    import hip
    C, N, cov, f, g, scale, gen = (case[k] for k in ("C", "N", "cov", "f", "g", "scale", "gen"))
    R = g.shape[0]
    mean = case["mean64"].float().cuda() if cov else None
    d = torch.randn(R, C, C, generator=torch.Generator().manual_seed(9))
    d = (d + d.transpose(1, 2)).cuda().contiguous()
    mask = (torch.randn(C, N, generator=torch.Generator().manual_seed(10)) - 0.2).cuda()
    mask[0, 0] = 0.0   # (zero counts as masked)
    base = torch.randn(C, N, generator=torch.Generator().manual_seed(11)).cuda()
    for accumulate in (False, True):
        start = base if accumulate else torch.full((C, N), float("nan"), device="cuda")
        plain, null, masked = start.clone(), start.clone(), start.clone()
        hip.gram_guided_bwd(d, f, g, scale, mean, plain, accumulate)
        hip.gram_guided_bwd_masked(d, f, g, scale, mean, null, accumulate, relu_mask=None)
        hip.gram_guided_bwd_masked(d, f, g, scale, mean, masked, accumulate, relu_mask=mask)
        torch.cuda.synchronize()
        assert torch.equal(null, plain), f"accumulate={accumulate}: a null mask changes bits"
        assert bool(plain.abs().sum() > 0)
        want = torch.where(mask <= 0, torch.zeros_like(plain), plain)
        assert torch.equal(masked, want), f"accumulate={accumulate}"
        assert bool((masked[mask <= 0] == 0).all()) and bool((mask <= 0).any()) and bool((mask > 0).any())


def test_predicate_and_refusal_before_any_launch():
    import hip
    L = hip.lib()
    assert hip.gram_guided_mse_ledger_supported(8, 512)   # VGG-19's worst case
    assert hip.gram_guided_mse_ledger_supported(8, 960) and not hip.gram_guided_mse_ledger_supported(8, 961)      # 8 x 120 x 4 = 3840; 8 x 136 x 4
    assert hip.gram_guided_mse_ledger_supported(1, 2816) and not hip.gram_guided_mse_ledger_supported(1, 2817)    # 990 x 4; 1035 x 4
    assert not hip.gram_guided_mse_ledger_supported(0, 64) and not hip.gram_guided_mse_ledger_supported(9, 64)
    R, C, N = 8, 1024, 4                                      # a shape maua_gram_guided_fwd takes, beyond the ledger bound
    assert L.maua_gram_guided_supported(R, C, N) == 1 and not hip.gram_guided_mse_ledger_supported(R, C)
    f, g = torch.rand(C, N).cuda(), torch.ones(R, N).cuda()
    scale, ls, gs = torch.full((R,), 0.01).cuda(), torch.ones(R).cuda(), torch.ones(R).cuda()
    gram, dmat, target = torch.full((R, C, C), 7.0).cuda(), torch.full((R, C, C), 7.0).cuda(), torch.zeros(R, C, C).cuda()
    led = hip.loss_ledger(1, 2, f.device)
    need = L.maua_gram_guided_workspace_bytes(R, C, N)
    ws = torch.zeros(need, dtype=torch.uint8).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    rc = L.maua_guided_gram_fwd_mse_ledger(P(f), P(g), P(scale), None, P(gram), None, R, C, N, 0, P(target), P(ls), P(gs), P(dmat), P(led), 1, P(ws),
                                           need, hip._stream())
    assert rc == -2 and b"partial sums" in L.maua_last_error()   # MAUA_E_UNSUPPORTED
    with pytest.raises(hip.HipError):
        hip.gram_guided_fwd_mse_ledger(f, g, scale, False, None, gram, None, target, dmat, ls, gs, led[0], 1, workspace=ws)
    # one null pointer at a time among the new arguments, on a supported shape: MAUA_E_INVAL
    C2 = 8
    for k in range(5):
        a = [P(target), P(ls), P(gs), P(dmat), P(led)]
        a[k] = None
        assert L.maua_guided_gram_fwd_mse_ledger(P(f), P(g), P(scale), None, P(gram), None, R, C2, N, 0, *a, 1, P(ws), need, hip._stream()) == -1, k
    torch.cuda.synchronize()
    assert bool((gram == 7).all()) and bool((dmat == 7).all()) and not bool(ws.any()) and not bool(led.any())
