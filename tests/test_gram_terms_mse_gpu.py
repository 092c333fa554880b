"""The shift and mirror terms' fused finish and masked backward (csrc/gram_shift.hip: maua_shift_gram_fwd_mse_ledger,
maua_shift_gram_bwd_masked; csrc/gram_flip.hip: maua_flip_gram_fwd_mse_ledger, maua_flip_gram_bwd_masked) against the plain kernels (bit for
bit) and fp64 (tests/shift_restatement.py, tests/flip_restatement.py).

Shapes (C, H, W): (3, 5, 7) - less than one stage; (70, 9, 33) - a plane that ends inside a stage, a ragged channel tile; (130, 20, 35) -
three channel tiles and a y offset beyond the backward kernel's 256-pixel tile; (450, 4, 18) with 16 shifts / 4 mirrors - eight channel
tiles, where the shifts' finishing launch has to take 4 partial sums per tile pair instead of 16 (16 x 64 x 16 would not fit one ledger
record; the 4 x 36 pairs of the mirrors still take 16).  Mirrors with and without `mean`, shifts too (the kernel centres on whatever means
it is given).  The second term of every call has loss_scale = grad_scale = 0.  Bars: D against fp64 at 2e-5 rel-L2 (TOL of
tests/test_gram_shift_gpu.py; D is a difference of two matrices, so the targets lie about a matrix norm away from the Gram matrices and the
bar is relative to a quantity of the operands' size), the loss at 1e-5 relative (the per-slot loss bar), the masked backward at 2e-5."""
import pytest
import torch

import flip_restatement as fr
import shift_restatement as sr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
TOL_LOSS = 1e-5
X, Y = 0, 1
SHIFTS = {(3, 5, 7): [(X, 4), (Y, 4)], (70, 9, 33): [(X, 4), (X, 16), (Y, 4)], (130, 20, 35): [(X, 4), (Y, 4), (X, 16), (Y, 16)],
          (450, 4, 18): [(X, d) for d in range(1, 14)] + [(Y, d) for d in (1, 2, 3)]}
KINDS = {(3, 5, 7): [fr.LR, fr.UD, fr.ROT180], (70, 9, 33): [fr.LR, fr.UD, fr.ROT180], (130, 20, 35): [fr.LR, fr.UD, fr.ROT180],
         (450, 4, 18): [fr.LR, fr.UD, fr.ROT180, fr.LR]}
PARAMS = [(which, chw, cov) for which in ("shift", "flip") for chw in SHIFTS for cov in (False, True)]


def per_pair(terms, pairs):
    return max(q for q in (4, 8, 16) if terms * pairs * q <= 4096)


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-C{p[1][0]}-{p[1][1]}x{p[1][2]}-{'cov' if p[2] else 'gram'}")
def case(request):
    which, (C, H, W), cov = request.param
    gen = torch.Generator().manual_seed(91 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    f64 = f.double()
    nt = (C + 63) // 64
    if which == "shift":
        terms = SHIFTS[(C, H, W)]
        scales = [1.0 / (C * (H * (W - d) if a == X else (H - d) * W)) for a, d in terms]
        g64 = torch.stack([sr.shifted_gram(f64, a, d, cov) for a, d in terms])
        t = torch.randn(len(terms), C, C, generator=gen, dtype=torch.float64)  # (not symmetric: a shifted product is not)
        pairs = nt * nt
    else:
        terms = KINDS[(C, H, W)]
        scales = [1.0 / (C * H * W)] * len(terms)
        g64 = torch.stack([fr.mirrored_gram(f64, k, cov) for k in terms])
        g64 = (g64 + g64.transpose(1, 2)) / 2
        t = torch.randn(len(terms), C, C, generator=gen, dtype=torch.float64)
        t = t + t.transpose(1, 2)  # (a captured target is a mirrored Gram matrix: symmetric)
        pairs = nt * (nt + 1) // 2
    target64 = g64 + t * (g64.norm() / 4 / (C + 1))
    K = len(terms)
    ls = [0.5 / (C * C) / (k + 1) for k in range(K)]
    gs = [3.0 / (C * C) / (k + 1) for k in range(K)]
    ls[1] = gs[1] = 0.0
    return dict(which=which, C=C, H=H, W=W, cov=cov, f=f.cuda(), f64=f64, mean=f64.mean((1, 2)).float().cuda() if cov else None, terms=terms,
                scales=scales, g64=g64, target=target64.float().cuda(), ls=ls, gs=gs, pairs=pairs)


def api(which):
    import hip
    if which == "shift":
        return hip.gram_shift_fwd, hip.gram_shift_fwd_mse_ledger, hip.gram_shift_bwd, hip.gram_shift_bwd_masked, hip.gram_shift_mse_ledger_supported
    return hip.gram_flip_fwd, hip.gram_flip_fwd_mse_ledger, hip.gram_flip_bwd, hip.gram_flip_bwd_masked, hip.gram_flip_mse_ledger_supported


def test_fused_forward_against_the_plain_forward_and_fp64(case):
    import hip
    which, C, f, mean, terms, scales, target, ls, gs = (case[k] for k in ("which", "C", "f", "mean", "terms", "scales", "target", "ls", "gs"))
    fwd, fused, _, _, supported = api(which)
    K = len(terms)
    assert supported(K, C)
    plain = fwd(f, terms, scales, mean)
    slots, slot = 3, 1
    runs = []
    for _ in range(2):
        led = hip.loss_ledger(1, slots, f.device)
        gram = torch.full((K, C, C), float("nan"), device="cuda")
        dmat = torch.full((K, C, C), float("nan"), device="cuda")
        fused(f, terms, scales, mean, gram, target, dmat, ls, gs, led[0], slot)
        record = led[0, slot].clone()
        losses, total = torch.zeros(1, slots, device="cuda"), torch.zeros(1, device="cuda")
        exact = torch.zeros(1, slots, dtype=torch.float64, device="cuda")
        hip.loss_ledger_sum(led, losses, total, exact)
        torch.cuda.synchronize()
        runs.append((gram, dmat, record, losses, exact))
    (gram, dmat, record, losses, exact), second = runs
    for a, b in zip(runs[0], second):
        assert torch.equal(a, b), "two runs differ"
    assert torch.equal(gram, plain), "gram: not the bits of the plain forward"
    q = per_pair(K, case["pairs"])
    assert (q == 4) == (which == "shift" and C == 450), q  # the case that must take fewer partial sums per tile pair
    assert float(record[1]) == 1.0 and int(record[0]) == q * K * case["pairs"]
    assert not bool(record[2 + int(record[0]):].any()), "partial sums beyond the record's count"
    assert not bool(led[0, [0, 2]].any()), "a neighbouring record was written"
    t64, g64 = target.double().cpu(), case["g64"]
    assert not bool(dmat[1].any()), "term with grad_scale = 0: D is not exact zeros"
    for k in range(K):
        if which == "flip":
            assert torch.equal(dmat[k], dmat[k].t()), f"D of mirror {k} is not bit-symmetric"
        if k == 1:
            continue
        e = rel_l2(dmat[k].cpu(), gs[k] * (g64[k] - t64[k]))
        print(f"  D[{k}] rel-L2 {e:.3e}")
        assert e <= TOL, (k, e)
    want = sum(ls[k] * float((g64[k] - t64[k]).pow(2).sum()) for k in range(K))  # (ls[1] = 0: term 1 contributes nothing)
    got = float(exact[0, slot])
    print(f"  loss {got:.9e} (fp64 {want:.9e}), fp32 slot {float(losses[0, slot]):.9e}")
    assert abs(got - want) <= TOL_LOSS * abs(want)
    assert abs(float(losses[0, slot]) - want) <= TOL_LOSS * abs(want)
    assert float(total[0]) == float(losses[0, slot])
    # term 1 with a NaN target: nothing of it reaches the loss, and its D stays exact zeros (both scales 0)
    bad = target.clone()
    bad[1] = float("nan")
    led = hip.loss_ledger(1, slots, f.device)
    fused(f, terms, scales, mean, gram, bad, dmat, ls, gs, led[0], slot)
    torch.cuda.synchronize()
    assert torch.equal(led[0, slot], record) and not bool(dmat[1].any())


def test_masked_backward(case):
    which, C, H, W, cov, f, mean, terms, scales = (case[k] for k in ("which", "C", "H", "W", "cov", "f", "mean", "terms", "scales"))
    _, _, bwd, bwd_masked, _ = api(which)
    K = len(terms)
    d = torch.randn(K, C, C, generator=torch.Generator().manual_seed(9))  # as given: not symmetric
    mask = (torch.randn(C, H, W, generator=torch.Generator().manual_seed(10)) - 0.2).cuda()
    mask[0, 0, 0] = 0.0   # (zero counts as masked)
    d64 = [m.double() for m in d]  # (both restatements apply 1 / (C n) themselves: `scales` here)
    if which == "shift":  # the gradient with respect to X = f - mean: no mean correction
        want64 = sr.shift_backward(sr.centred(case["f64"], cov), terms, d64, False)
    else:
        want64 = fr.flip_backward(case["f64"], terms, d64, cov)
    # (of the size of what is added: masked - base is then exact to rounding)
    base = (torch.randn(C, H, W, generator=torch.Generator().manual_seed(11)) * float(want64.abs().max())).cuda()
    d = d.cuda().contiguous()
    for accumulate in (False, True):
        start = base if accumulate else torch.full((C, H, W), float("nan"), device="cuda")
        plain, null, masked = start.clone(), start.clone(), start.clone()
        bwd(d, f, terms, scales, mean, plain, accumulate)
        bwd_masked(d, f, terms, scales, mean, null, accumulate, relu_mask=None)
        bwd_masked(d, f, terms, scales, mean, masked, accumulate, relu_mask=mask)
        torch.cuda.synchronize()
        assert torch.equal(null, plain), f"accumulate={accumulate}: a null mask changes bits"
        assert not bool(torch.isnan(plain).any()) and bool(plain.abs().sum() > 0)
        want = torch.where(mask <= 0, torch.zeros_like(plain), plain)
        assert torch.equal(masked, want), f"accumulate={accumulate}"
        assert bool((masked[mask <= 0] == 0).all()) and bool((mask <= 0).any()) and bool((mask > 0).any())
        got = masked.double().cpu() - (base.double().cpu() * (mask > 0).cpu() if accumulate else 0)
        e = rel_l2(got, want64 * (mask > 0).cpu())
        print(f"  accumulate={accumulate}: masked gx rel-L2 {e:.3e}")
        assert e <= TOL, (accumulate, e)


def test_refusal_before_any_launch():
    import hip
    L = hip.lib()
    C, H, W = 2049, 1, 4  # a shape both plain forwards take, beyond the ledger bound of a single term
    f = torch.rand(C, H, W).cuda()
    gram, dmat, target = torch.full((1, C, C), 7.0).cuda(), torch.full((1, C, C), 7.0).cuda(), torch.zeros(1, C, C).cuda()
    led = hip.loss_ledger(1, 2, f.device)
    assert L.maua_gram_shift_supported(1, C, H, W) == 1 and not hip.gram_shift_mse_ledger_supported(1, C)
    ws = torch.zeros(hip.gram_shift_workspace_bytes(1, C, H, W), dtype=torch.uint8).cuda()
    with pytest.raises(hip.HipError, match="partial sums"):
        hip.gram_shift_fwd_mse_ledger(f, [(X, 1)], [1.0], None, gram, target, dmat, [1.0], [1.0], led[0], 1, workspace=ws)
    C2 = 2881
    assert L.maua_gram_flip_supported(1, C2, H, W) == 1 and not hip.gram_flip_mse_ledger_supported(1, C2)
    with pytest.raises(hip.HipError, match="partial sums"):
        hip.gram_flip_fwd_mse_ledger(torch.rand(C2, H, W).cuda(), [fr.LR], [1.0], None, torch.zeros(1, C2, C2).cuda(), torch.zeros(1, C2, C2).cuda(),
                                     torch.zeros(1, C2, C2).cuda(), [1.0], [1.0], led[0], 1)
    torch.cuda.synchronize()
    assert bool((gram == 7).all()) and bool((dmat == 7).all()) and not bool(ws.any()) and not bool(led.any())
