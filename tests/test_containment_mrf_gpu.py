"""Containment of the MRF patch-matching entry points (csrc/mrf.hip): their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_feat_hist_gpu.py does:
importing this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of
the whole suite; this module's name sorts after test_containment_gpu.py (as tests/test_containment_gram_flip_gpu.py does), so every case
runs once, below, under the same checks - the two guard fills (0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of
everything written intact, every defined element written, the workspace really used), the declared entry points called, and bit equality
of outputs, state and workspace between the fills.

What could go wrong here: the match stages 16 channels x 256 queries and 16 channels x 128 patches whatever the shape, so a padded query
(Q = 1, 15, 217, 594 against tiles of 256), a padded patch (P = 1, 28, 290, 209 against tiles of 128) or a channel past C (2, 3, 70, 130
against blocks of 16) that formed an address would read beside F or S, and one that was compared could win with whatever it read - the bits
would then differ between the fills; the last tap of the last query and of the last listed patch end exactly at the end of F and S; the
gather passes read nn at up to nine queries around a pixel, those outside the query grid must not be formed.  The workspace is exactly
maua_mrf_workspace_bytes and the state exactly maua_mrf_state_bytes.  Value bar: TOL of tests/test_kernels_gpu.py (2e-5), as in
tests/test_mrf_gpu.py, with the restatement pinned to the decisions read back."""
import pytest
import torch

import mrf_restatement as mr
import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5
SHAPES = [dict(C=C, H=H, W=W, Hs=Hs, Ws=Ws, stride=stride)
          for C, H, W, Hs, Ws, stride in ((2, 3, 3, 3, 3, 1), (3, 5, 7, 6, 9, 1), (70, 9, 33, 12, 31, 1), (130, 20, 35, 23, 40, 2))]


@cg.case(("maua_mrf_bank", "maua_mrf_fwd", "maua_mrf_bwd"), SHAPES)
def mrf(c, C, H, W, Hs, Ws, stride):
    gen = torch.Generator().manual_seed(73 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(torch.randn(C, Hs, Ws, generator=gen) + 0.3)
    s, origin, inv_r, _ = mr.build_bank([s], stride, 1 << 20)
    P, Q = origin.numel(), (H - 2) * (W - 2)
    assert int(origin[-1]) + 2 * Ws + 2 == Hs * Ws - 1 or stride > 1  # (stride 1: the last patch ends with the map)
    assert c.L.maua_mrf_supported(C, H, W, Hs, Ws, P) == 1
    fin, sin, oin = c.inp(f), c.inp(s), c.inp(origin)
    inv = c.out("inv", P)
    c.ok(c.L.maua_mrf_bank(cg.P(sin), cg.P(oin), cg.P(inv), C, Hs, Ws, P, c.S()), "maua_mrf_bank")
    torch.cuda.synchronize()
    assert float(((inv.cpu().double() - inv_r.double()).abs() / inv_r.double()).max()) <= 2.0 ** -23
    iin = c.inp(inv.clone())  # the consumer reads a copy between input guards
    ws = c.used(c.ws("workspace", c.L.maua_mrf_workspace_bytes(C, H, W, Hs, Ws, P)))
    state = c.ws("state", c.L.maua_mrf_state_bytes(H, W))
    loss = c.out("loss", 1)
    c.ok(c.L.maua_mrf_fwd(cg.P(fin), cg.P(sin), cg.P(oin), cg.P(iin), cg.P(state), cg.P(loss), C, H, W, Hs, Ws, P, cg.P(ws), cg.nb(ws), c.S()),
         "maua_mrf_fwd")
    torch.cuda.synchronize()
    nn = state.view(torch.int32)[:Q].cpu()
    sc = mr.scores(f, s, origin, inv_r)
    best, margin = mr.margins(sc)
    assert int(nn.min()) >= 0 and int(nn.max()) < P
    assert bool((sc[torch.arange(Q), nn.long()] >= (1 - TOL) * best).all())
    assert torch.equal(nn.long()[margin > TOL], mr.nearest(sc)[margin > TOL])
    c.check("best", state.view(torch.float32)[Q:], best, TOL)
    c.check("loss", loss, mr.loss(f, s, origin, nn).reshape(1), TOL)
    # backward, both accumulate forms: written with upstream NULL, accumulated with a device scalar
    want = mr.gather_gradient(f, s, origin, nn)
    up, coef = -1.75, 0.37
    want_acc = mr.gather_gradient(f, s, origin, nn, coef=coef * up)
    base = torch.randn(C, H, W, generator=gen) * float(want_acc.abs().max())
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    upstream = c.inp(torch.tensor([up]))
    c.ok(c.L.maua_mrf_bwd(cg.P(fin), cg.P(sin), cg.P(oin), cg.P(state), None, 2.0 / (9 * C * Q), cg.P(gx), C, H, W, Hs, Ws, P, 0, c.S()),
         "maua_mrf_bwd")
    c.ok(c.L.maua_mrf_bwd(cg.P(fin), cg.P(sin), cg.P(oin), cg.P(state), cg.P(upstream), coef, cg.P(acc), C, H, W, Hs, Ws, P, 1, c.S()),
         "maua_mrf_bwd")
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
