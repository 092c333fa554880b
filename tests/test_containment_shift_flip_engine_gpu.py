"""Containment of the shift and mirror terms' engine entry points (csrc/gram_shift.hip: maua_shift_gram_fwd_mse_ledger,
maua_shift_gram_bwd_masked; csrc/gram_flip.hip: maua_flip_gram_fwd_mse_ledger, maua_flip_gram_bwd_masked): their cases in the table of
tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_guided_engine_gpu.py does:
importing this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of
the whole suite (this module's name sorts before that one's and after test_containment_gpu.py), so every case runs once, below, under the
same checks - the two guard fills (0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of everything written intact,
every defined element written, the workspace really used), the declared entry points called, and bit equality of outputs and workspace
between the fills.

Shapes, shifts and kinds: those of tests/test_containment_shift_gpu.py and tests/test_containment_gram_flip_gpu.py (less than one stage; a
plane that ends inside a stage with a ragged channel tile; three channel tiles with a y offset beyond the backward kernel's 256-pixel
tile), centred and not.  The workspace is exactly maua_gram_shift_workspace_bytes / maua_gram_flip_workspace_bytes, the ledger exactly
maua_loss_ledger_bytes(1, 3) with the record in the middle slot: the records on either side must keep their bits.  The last term of every
case has grad_scale 0 (its D must be WRITTEN as zeros), the first loss_scale 0.  Value bar: 2e-5 for contractions, as there."""
import ctypes

import pytest
import torch

import flip_restatement as fr
import shift_restatement as sr
import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)
from test_containment_gram_flip_gpu import KINDS
from test_containment_gram_flip_gpu import SHAPES as FLIP_SHAPES
from test_containment_shift_gpu import SHAPES as SHIFT_SHAPES
from test_containment_shift_gpu import SHIFTS, X

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5


def _doubles(vals):
    return (ctypes.c_double * len(vals))(*vals)


def _coefficients(K, C):
    ls = [0.0] + [0.5 / (C * C) / (k + 1) for k in range(1, K)]
    gs = [3.0 / (C * C) / (k + 1) for k in range(K - 1)] + [0.0]
    return ls, gs


def _ledger(c, slots=3):
    nbytes = c.L.maua_loss_ledger_bytes(1, slots)
    led = c.inout("ledger", torch.zeros(1, slots, nbytes // 8 // slots, dtype=torch.float64), kind="raw")
    assert led.numel() * 8 == nbytes
    c.only(led, lambda m: m[0, 1])
    return led


def _loss_check(c, led, diff, ls, slots=3):
    losses, totals = c.inout("losses", torch.zeros(1, slots)), c.out("totals", 1)
    c.only(losses, lambda m: m[0, 1])
    c.hip.loss_ledger_sum(led, losses, totals)
    torch.cuda.synchronize()
    c.check("loss", losses[0, 1:2], sum(ls[k] * (diff[k] ** 2).sum() for k in range(len(ls))).reshape(1), TOL)


@cg.case(("maua_shift_gram_fwd_mse_ledger", "maua_shift_gram_bwd_masked"), SHIFT_SHAPES)
def shift_engine(c, C, H, W, center):
    gen = torch.Generator().manual_seed(47 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    shifts = SHIFTS[(C, H, W)]
    S = len(shifts)
    f64 = f.double()
    mean64 = f64.mean((1, 2))
    scale = [1.0 / (C * (H * (W - d) if a == X else (H - d) * W)) for a, d in shifts]
    axes, deltas = (ctypes.c_int * S)(*[a for a, _ in shifts]), (ctypes.c_int * S)(*[d for _, d in shifts])
    gram64 = torch.stack([sr.shifted_gram(f64, a, d, bool(center)) for a, d in shifts])
    target = (gram64 + torch.randn(S, C, C, generator=gen, dtype=torch.float64) * (gram64.norm() / 4 / (C + 1))).float()
    ls, gs = _coefficients(S, C)
    assert c.L.maua_shift_gram_mse_ledger_supported(S, C) == 1
    fin = c.inp(f)
    mean_in = cg.P(c.inp(mean64.float())) if center else None
    led = _ledger(c)
    ws = c.used(c.ws("workspace", c.L.maua_gram_shift_workspace_bytes(S, C, H, W)))
    gram, dmat = c.out("gram", S, C, C), c.out("dmat", S, C, C)
    c.ok(c.L.maua_shift_gram_fwd_mse_ledger(cg.P(fin), mean_in, axes, deltas, _doubles(scale), cg.P(gram), S, C, H, W, cg.P(c.inp(target)),
                                            _doubles(ls), _doubles(gs), cg.P(dmat), cg.P(led), 1, cg.P(ws), cg.nb(ws), c.S()),
         "maua_shift_gram_fwd_mse_ledger")
    torch.cuda.synchronize()
    diff = gram64 - target.double()
    for s in range(S):
        c.check(f"gram[{s}]", gram[s], gram64[s], TOL)
        if gs[s] == 0:
            assert not bool(dmat[s].any())
        else:
            c.check(f"dmat[{s}]", dmat[s], gs[s] * diff[s], TOL)
    _loss_check(c, led, diff, ls)
    # masked backward, both accumulate forms; D is random and not symmetric
    dm = torch.randn(S, C, C, generator=gen)
    mask = torch.randn(C, H, W, generator=gen)
    x64 = f64 - mean64[:, None, None] if center else f64
    want = sr.shift_backward(x64, shifts, [m.double() for m in dm], False) * (mask > 0)
    base = torch.randn(C, H, W, generator=gen) * float(want.abs().max())
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    din, min_ = c.inp(dm), c.inp(mask)
    for out, accumulate in ((gx, 0), (acc, 1)):
        c.ok(c.L.maua_shift_gram_bwd_masked(cg.P(din), cg.P(fin), mean_in, axes, deltas, _doubles(scale), cg.P(min_), cg.P(out), S, C, H, W,
                                            accumulate, c.S()), "maua_shift_gram_bwd_masked")
    c.check("gx", gx, want, TOL)
    c.check("gx accumulated", acc.double().cpu() - (base * (mask > 0)).double(), want, TOL)
    torch.cuda.synchronize()
    assert not bool(gx[(mask <= 0).cuda()].any()) and not bool(acc[(mask <= 0).cuda()].any())


@cg.case(("maua_flip_gram_fwd_mse_ledger", "maua_flip_gram_bwd_masked"), FLIP_SHAPES)
def flip_engine(c, C, H, W, center):
    gen = torch.Generator().manual_seed(53 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    M = len(KINDS)
    f64 = f.double()
    mean64 = f64.mean((1, 2))
    kinds = (ctypes.c_int * M)(*KINDS)
    scale = [1.0 / (C * H * W)] * M
    gram64 = torch.stack([fr.mirrored_gram(f64, k, bool(center)) for k in KINDS])
    gram64 = (gram64 + gram64.transpose(1, 2)) / 2
    t = torch.randn(M, C, C, generator=gen, dtype=torch.float64)
    target = (gram64 + (t + t.transpose(1, 2)) * (gram64.norm() / 4 / (C + 1))).float()
    ls, gs = _coefficients(M, C)
    assert c.L.maua_flip_gram_mse_ledger_supported(M, C) == 1
    fin = c.inp(f)
    mean_in = cg.P(c.inp(mean64.float())) if center else None
    led = _ledger(c)
    ws = c.used(c.ws("workspace", c.L.maua_gram_flip_workspace_bytes(M, C, H, W)))
    gram, dmat = c.out("gram", M, C, C), c.out("dmat", M, C, C)
    c.ok(c.L.maua_flip_gram_fwd_mse_ledger(cg.P(fin), mean_in, kinds, _doubles(scale), cg.P(gram), M, C, H, W, cg.P(c.inp(target)), _doubles(ls),
                                           _doubles(gs), cg.P(dmat), cg.P(led), 1, cg.P(ws), cg.nb(ws), c.S()), "maua_flip_gram_fwd_mse_ledger")
    torch.cuda.synchronize()
    diff = gram64 - target.double()
    for m in range(M):
        assert torch.equal(gram[m], gram[m].t()) and torch.equal(dmat[m], dmat[m].t())
        c.check(f"gram[{m}]", gram[m], gram64[m], TOL)
        if gs[m] == 0:
            assert not bool(dmat[m].any())
        else:
            c.check(f"dmat[{m}]", dmat[m], gs[m] * diff[m], TOL)
    _loss_check(c, led, diff, ls)
    # masked backward, both accumulate forms; D is random and not symmetric
    dm = torch.randn(M, C, C, generator=gen)
    mask = torch.randn(C, H, W, generator=gen)
    want = fr.flip_backward(f64, KINDS, [m.double() for m in dm], bool(center)) * (mask > 0)
    base = torch.randn(C, H, W, generator=gen) * float(want.abs().max())
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    din, min_ = c.inp(dm), c.inp(mask)
    for out, accumulate in ((gx, 0), (acc, 1)):
        c.ok(c.L.maua_flip_gram_bwd_masked(cg.P(din), cg.P(fin), mean_in, kinds, _doubles(scale), cg.P(min_), cg.P(out), M, C, H, W, accumulate,
                                           c.S()), "maua_flip_gram_bwd_masked")
    c.check("gx", gx, want, TOL)
    c.check("gx accumulated", acc.double().cpu() - (base * (mask > 0)).double(), want, TOL)
    torch.cuda.synchronize()
    assert not bool(gx[(mask <= 0).cuda()].any()) and not bool(acc[(mask <= 0).cuda()].any())


CASES = cg.TABLE[FIRST:]


@pytest.mark.parametrize("entry", CASES, ids=lambda e: e.id)
def test_contained(recorded, entry):  # noqa: F811
    hip, called = recorded
    called.clear()
    runs = []
    for fill in (0x00, 0xFF):
        c = cg.Ctx(hip, fill)
        try:
            entry.fn(c, **entry.params)
            runs.append(c.finish())
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):   # a faulted device: nothing more is started on it
                pytest.exit(f"{entry.id}: {e}", returncode=3)
            raise
    missing = set(entry.entries) - called
    assert not missing, f"the case declares entry points it did not call: {sorted(missing)}"
    (bits0, sizes), (bits1, _) = runs
    assert bits0.keys() == bits1.keys()
    differ = [k for k in bits0 if not torch.equal(bits0[k], bits1[k])]
    assert not differ, f"results depend on what lies beyond the inputs (guards of 0x00 against 0xFF): {differ}"
    print(f"{entry.id}: {', '.join(sizes)}: guards intact, bits equal under both fills")
