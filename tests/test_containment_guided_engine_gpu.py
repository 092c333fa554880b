"""Containment of the guided layer's engine entry points (csrc/gram_guided.hip: maua_guided_gram_fwd_mse_ledger, maua_guided_gram_bwd_masked):
their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_guided_gpu.py does: importing
this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of the whole
suite; this module's name sorts after test_containment_gpu.py, so every case runs once, below, under the same checks - the two guard
fills (0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of everything written intact, every defined element
written, the workspace really used), the declared entry points called, and bit equality of outputs and workspace between the fills.

Shapes and regions: those of tests/test_containment_guided_gpu.py (channels that are no multiple of the 64-channel tile, planes that end
inside a stage and inside the backward kernel's tile, one plane smaller than a stage; a hard mask, a soft one, one without mass - whose
Gram AND D matrices must be WRITTEN as zeros).  The workspace is exactly maua_gram_guided_workspace_bytes, the ledger exactly
maua_loss_ledger_bytes(1, 3) with the record in the middle slot: the records on either side must keep their bits.  Value bar: 2e-5 for
contractions, as there."""
import pytest
import torch

import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)
from test_containment_guided_gpu import SHAPES, TOL, _inputs, _reference

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)


@cg.case(("maua_guided_gram_fwd_mse_ledger", "maua_guided_gram_bwd_masked"), SHAPES)
def guided_engine(c, C, N, center):
    hip = c.hip
    f, guides, gen = _inputs(C, N)
    R = guides.shape[0]
    mass64, scale64, gram64, mean64 = _reference(f, guides, center)
    assert c.L.maua_guided_gram_mse_ledger_supported(R, C) == 1
    scale = scale64.float()
    t = torch.randn(R, C, C, generator=gen, dtype=torch.float64)
    target = (gram64 + (t + t.transpose(1, 2)) * (gram64.norm() / 4 / (C + 1))).float()
    ls = torch.tensor([0.5 / (C * C), 0.25 / (C * C), 0.0])
    gs = torch.tensor([3.0 / (C * C), 1.5 / (C * C), 2.0 / (C * C)])
    slots, slot = 3, 1
    nbytes = c.L.maua_loss_ledger_bytes(1, slots)
    led = c.inout("ledger", torch.zeros(1, slots, nbytes // 8 // slots, dtype=torch.float64), kind="raw")
    assert led.numel() * 8 == nbytes
    c.only(led, lambda m: m[0, slot])
    ws = c.used(c.ws("workspace", c.L.maua_gram_guided_workspace_bytes(R, C, N)))
    gram, dmat = c.out("gram", R, C, C), c.out("dmat", R, C, C)
    mean = c.out("mean", R, C) if center else None
    c.ok(c.L.maua_guided_gram_fwd_mse_ledger(
        cg.P(c.inp(f)), cg.P(c.inp(guides)), cg.P(c.inp(scale)), cg.P(c.inp(mass64)) if center else None, cg.P(gram), cg.P(mean), R, C, N, center,
        cg.P(c.inp(target)), cg.P(c.inp(ls)), cg.P(c.inp(gs)), cg.P(dmat), cg.P(led), slot, cg.P(ws), cg.nb(ws), c.S()), "maua_guided_gram_fwd_mse_ledger")
    losses, totals = c.inout("losses", torch.zeros(1, slots)), c.out("totals", 1)
    c.only(losses, lambda m: m[0, slot])
    hip.loss_ledger_sum(led, losses, totals)
    torch.cuda.synchronize()
    diff = gram64 - target.double()
    for r in range(R):
        assert torch.equal(gram[r], gram[r].t()) and torch.equal(dmat[r], dmat[r].t())
        if scale64[r] == 0:
            assert not bool(gram[r].any()) and not bool(dmat[r].any()) and (mean is None or not bool(mean[r].any()))
        else:
            c.check(f"gram[{r}]", gram[r], gram64[r], TOL)
            c.check(f"dmat[{r}]", dmat[r], float(gs[r].double()) * diff[r], TOL)
    c.check("loss", losses[0, slot:slot + 1], sum(float(ls[r].double()) * (diff[r] ** 2).sum() for r in range(R)).reshape(1), TOL)
    # masked backward, both accumulate forms; mask and means are read from copies between input guards
    d = torch.randn(R, C, C, generator=gen)
    d = d + d.transpose(1, 2)
    mask = torch.randn(C, N, generator=gen)
    want = sum(float(scale64[r]) * (d[r].double() @ (f.double() - mean64[r][:, None])) * (guides[r].double() ** 2)[None] for r in range(R))
    want = want * (mask > 0)
    base = torch.randn(C, N, generator=gen) * float(want.abs().max())
    mean_in = cg.P(c.inp(mean64.float())) if center else None
    gf, acc = c.out("gf", C, N), c.inout("gf_acc", base)
    for out, accumulate in ((gf, 0), (acc, 1)):
        c.ok(c.L.maua_guided_gram_bwd_masked(cg.P(c.inp(d)), cg.P(c.inp(f)), cg.P(c.inp(guides)), cg.P(c.inp(scale)), mean_in, cg.P(c.inp(mask)),
                                             cg.P(out), R, C, N, accumulate, c.S()), "maua_guided_gram_bwd_masked")
    c.check("gf", gf, want, TOL)
    c.check("gf accumulated", acc.double().cpu() - (base * (mask > 0)).double(), want, TOL)
    torch.cuda.synchronize()
    assert not bool(gf[(mask <= 0).cuda()].any()) and not bool(acc[(mask <= 0).cuda()].any())


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
