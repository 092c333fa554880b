"""Containment of the sliced Wasserstein entry points (csrc/swd.hip): their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_mrf_gpu.py does: importing
this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of the whole
suite; this module's name sorts after test_containment_gpu.py, so every case runs once, below, under the same checks - the two guard fills
(0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of everything written intact, every defined element written,
the workspace really used), the declared entry points called, and bit equality of outputs, state and workspace between the fills.

What could go wrong here: both products stage 16 values of K x 256 pixels and 16 x 32, 16 x 64 or 16 x 128 values of the directions whatever
the shape, so a pixel past N (35, 297, 700, 256 against tiles of 256), a row past D or C (5, 70, 64, 96, 3, 130 against blocks of 32, 64 and 128) or
a k past C or D (3, 70, 130 against stages of 16) that formed an address would read beside F, V or G, and a padded pixel that entered a
row's (min, max) would change lo or hi - a 0 where every projection is positive; the store of a padded row or pixel would write beside P or
gx; the residual pass writes over P through 16-byte quads with scalar heads and tails (rows of 35, 297 and 700 elements start off 16-byte
boundaries).  The workspace is exactly maua_swd_workspace_bytes and the state exactly maua_swd_state_bytes; P is an output of the first
call and an in-out buffer of the second.  Value bar: TOL of tests/test_kernels_gpu.py (2e-5), as in tests/test_swd_gpu.py, with the
restatement applied to the P read back."""
import pytest
import torch

import feat_hist_restatement as hr
import swd_restatement as wr
import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5
SHAPES = [dict(C=C, D=D, H=H, W=W, bins=bins, knots=knots)
          for (C, D, H, W), (bins, knots) in (((3, 5, 5, 7), (16, 2)), ((70, 70, 9, 33), (256, 1024)), ((130, 64, 20, 35), (1024, 64)),
                                              ((64, 96, 16, 16), (256, 1024)))]


@cg.case(("maua_swd_project", "maua_swd_match", "maua_swd_bwd"), SHAPES)
def swd(c, C, D, H, W, bins, knots):
    gen = torch.Generator().manual_seed(79 + C + D + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(2 * torch.randn(C, H + 3, W + 5, generator=gen) + 1)
    v = wr.directions(C, D, 1, 0).clone()
    v[D // 2] = 0.0
    table = wr.table(s, v, knots).float()
    t64 = table.double()
    N = H * W
    assert c.L.maua_swd_supported(C, D, H, W, bins, knots) == 1
    fin, vin, vtin, tin = c.inp(f), c.inp(v), c.inp(v.t().contiguous()), c.inp(table)
    ws = c.used(c.ws("workspace", c.L.maua_swd_workspace_bytes(C, D, H, W, bins, knots)))
    state = c.ws("state", c.L.maua_swd_state_bytes(D, bins))
    proj, plain = c.out("proj", D, H, W), c.out("proj_plain", D, H, W)
    loss = c.out("loss", 1)
    c.ok(c.L.maua_swd_project(cg.P(fin), cg.P(vin), cg.P(plain), None, C, D, H, W, 0, None, 0, c.S()), "maua_swd_project")
    c.ok(c.L.maua_swd_project(cg.P(fin), cg.P(vin), cg.P(proj), cg.P(state), C, D, H, W, bins, cg.P(ws), cg.nb(ws), c.S()), "maua_swd_project")
    torch.cuda.synchronize()
    p = proj.cpu().clone()
    assert torch.equal(plain.cpu(), p)
    c.check("projection", p, wr.project(f, v), TOL)
    c.ok(c.L.maua_swd_match(cg.P(proj), cg.P(tin), cg.P(state), cg.P(loss), D, H, W, bins, knots, cg.P(ws), cg.nb(ws), c.S()), "maua_swd_match")
    torch.cuda.synchronize()
    lo_r, hi_r, cum_r = hr.state(p, bins)
    rec = state.view(torch.int32).reshape(D, bins + 3).cpu()
    ends = rec[:, :2].contiguous().view(torch.float32)
    assert torch.equal(ends[:, 0], torch.from_numpy(lo_r)) and torch.equal(ends[:, 1], torch.from_numpy(hi_r))
    assert torch.equal(rec[:, 2:].long(), torch.from_numpy(cum_r))
    c.check("loss", loss, hr.term(p.double(), t64, bins).reshape(1), TOL)
    c.check("G", proj, wr.residual(p, t64, bins), TOL)
    # backward, both accumulate forms: written with upstream NULL, accumulated with a device scalar
    want = wr.backward(p, v, t64, bins)
    up, coef = -1.75, 0.37
    want_acc = wr.backward(p, v, t64, bins, coef=coef, upstream=up)
    base = torch.randn(C, H, W, generator=gen) * float(want_acc.abs().max())
    gin = c.inp(proj.clone())  # the consumer reads a copy between input guards
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    upstream = c.inp(torch.tensor([up]))
    c.ok(c.L.maua_swd_bwd(cg.P(gin), cg.P(vtin), None, 2.0 / (D * N), cg.P(gx), C, D, H, W, 0, c.S()), "maua_swd_bwd")
    c.ok(c.L.maua_swd_bwd(cg.P(gin), cg.P(vtin), cg.P(upstream), coef, cg.P(acc), C, D, H, W, 1, c.S()), "maua_swd_bwd")
    c.check("gx", gx, want, TOL)
    c.check("gx accumulated", acc.double().cpu() - base.double(), want_acc, TOL)


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
