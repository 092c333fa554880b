"""Containment of the feature-histogram entry points (csrc/feat_hist.hip): their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_gram_flip_gpu.py does:
importing this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of
the whole suite.  The cases run below under the same checks - the two guard fills (0x00, 0xFF) around everything an entry point reads,
`Ctx.finish()` (guards of everything written intact, every defined element written, the workspace really used), the declared entry points
called, and bit equality of outputs, state and workspace between the fills.  This module's name sorts before test_containment_gpu.py, whose
parametrisation reads the table when that module is collected: in a run of the whole suite the four cases run there a second time (about a
second each); a run of this file alone runs them once.

What could go wrong here: the scalar head and tail around the 16-byte quads of a chunk (a quad formed one element early reads in front of
the plane, a tail formed from the wrong base reads behind F), the last chunk of a channel (3 elements of a 1024-element chunk at
(2, 257, 259)), the LDS staging of the table and of cum[0 .. bins] (bins + 1 entries), and the counters' zeroing - a value loaded and
multiplied by zero would still differ between the fills.  The workspace is exactly maua_feat_hist_workspace_bytes and the state exactly
maua_feat_hist_state_bytes.  Value bar: TOL of tests/test_kernels_gpu.py (2e-5), as in tests/test_feat_hist_gpu.py."""
import pytest
import torch

import feat_hist_restatement as hr
import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5
SHAPES = [dict(C=C, H=H, W=W, bins=bins, knots=knots)
          for (C, H, W), (bins, knots) in (((3, 5, 7), (16, 2)), ((70, 9, 33), (256, 1024)), ((130, 20, 35), (1024, 64)), ((2, 257, 259), (256, 1024)))]


@cg.case(("maua_feat_hist_fwd", "maua_feat_hist_bwd"), SHAPES)
def feat_hist(c, C, H, W, bins, knots):
    gen = torch.Generator().manual_seed(71 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    if C > 2:
        f[1] = 0.625
        f[C - 1] = 0.0
    table = hr.quantile_table(torch.relu(2 * torch.randn(C, H + 3, W + 5, generator=gen) + 1), knots)
    f64, t64 = f.double(), table.double()
    N = H * W
    assert c.L.maua_feat_hist_supported(C, H, W, bins, knots) == 1
    fin, tin = c.inp(f), c.inp(table)
    ws = c.used(c.ws("workspace", c.L.maua_feat_hist_workspace_bytes(C, H, W, bins, knots)))
    state = c.ws("state", c.L.maua_feat_hist_state_bytes(C, bins))
    loss = c.out("loss", 1)
    c.ok(c.L.maua_feat_hist_fwd(cg.P(fin), cg.P(tin), cg.P(state), cg.P(loss), C, H, W, bins, knots, cg.P(ws), cg.nb(ws), c.S()),
         "maua_feat_hist_fwd")
    torch.cuda.synchronize()
    lo_r, hi_r, cum_r = hr.state(f64, bins)
    rec = state.view(torch.int32).reshape(C, bins + 3).cpu()
    ends = rec[:, :2].contiguous().view(torch.float32)
    assert torch.equal(ends[:, 0], torch.from_numpy(lo_r)) and torch.equal(ends[:, 1], torch.from_numpy(hi_r))
    assert torch.equal(rec[:, 2:].long(), torch.from_numpy(cum_r))
    c.check("loss", loss, hr.term(f64, t64, bins).reshape(1), TOL)
    # backward, both accumulate forms: written with upstream NULL, accumulated with a device scalar
    want = hr.backward(f64, t64, bins)
    up, coef = -1.75, 0.37
    want_acc = want * (coef * up * C * N / 2.0)
    base = torch.randn(C, H, W, generator=gen) * float(want_acc.abs().max())
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    upstream = c.inp(torch.tensor([up]))
    c.ok(c.L.maua_feat_hist_bwd(cg.P(fin), cg.P(tin), cg.P(state), None, 2.0 / (C * N), cg.P(gx), C, H, W, bins, knots, 0, c.S()),
         "maua_feat_hist_bwd")
    c.ok(c.L.maua_feat_hist_bwd(cg.P(fin), cg.P(tin), cg.P(state), cg.P(upstream), coef, cg.P(acc), C, H, W, bins, knots, 1, c.S()),
         "maua_feat_hist_bwd")
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
