"""Containment of the mirrored Gram entry points (csrc/gram_flip.hip): their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_shift_gpu.py does: importing
this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of the whole
suite; this module's name sorts after test_containment_gpu.py, so every case runs once, below, under the same checks - the two guard
fills (0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of everything written intact, every defined element
written, the workspace really used), the declared entry points called, and bit equality of outputs and workspace between the fills.

The bit equality is the point here: the mirrored operand is read in descending address order, a quad at sigma(p) - 3 .. sigma(p), so an
off-by-one of the reversed 16-byte load reads in front of a row of F - in front of F itself for the first channel's last quad - and the
ragged last stage must not touch what lies behind the plane's end.  A position that were loaded and multiplied by zero would still differ
between the fills (0xFF bytes are NaNs), and F sits between guards of either fill.

Shapes (C, H, W): (3, 5, 7) - less than one stage, odd H and W, row ends inside the quads; (70, 9, 33) - a plane that ends inside a stage, a
ragged channel tile; (130, 20, 35) - three channel tiles, several backward pixel tiles.  All three kinds in one call, centred and not.  The
workspace is exactly maua_gram_flip_workspace_bytes.  Value bar: TOL of tests/test_kernels_gpu.py for contractions (2e-5), as in
tests/test_gram_flip_gpu.py."""
import ctypes

import pytest
import torch

import flip_restatement as fr
import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5
KINDS = [fr.LR, fr.UD, fr.ROT180]
SHAPES = [dict(C=C, H=H, W=W, center=center) for (C, H, W) in ((3, 5, 7), (70, 9, 33), (130, 20, 35)) for center in (0, 1)]


@cg.case(("maua_gram_flip_fwd", "maua_gram_flip_bwd"), SHAPES)
def gram_flip(c, C, H, W, center):
    gen = torch.Generator().manual_seed(43 + C + H + W)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    M = len(KINDS)
    f64 = f.double()
    mean64 = f64.mean((1, 2))
    kinds = (ctypes.c_int * M)(*KINDS)
    factors = (ctypes.c_double * M)(*[1.0 / (C * H * W)] * M)
    assert c.L.maua_gram_flip_supported(M, C, H, W) == 1
    fin = c.inp(f)
    mean_in = cg.P(c.inp(mean64.float())) if center else None
    # forward
    ws = c.used(c.ws("workspace", c.L.maua_gram_flip_workspace_bytes(M, C, H, W)))
    gram = c.out("gram", M, C, C)
    c.ok(c.L.maua_gram_flip_fwd(cg.P(fin), mean_in, kinds, factors, cg.P(gram), M, C, H, W, cg.P(ws), cg.nb(ws), c.S()), "maua_gram_flip_fwd")
    torch.cuda.synchronize()
    for m, k in enumerate(KINDS):
        c.check(f"gram[{('LR', 'UD', '180')[k]}]", gram[m], fr.mirrored_gram(f64, k, bool(center)), TOL)
        assert torch.equal(gram[m], gram[m].t())
    # backward, both accumulate forms; D is random and not symmetric
    dm = torch.randn(M, C, C, generator=gen)
    want = fr.flip_backward(f64, KINDS, [m.double() for m in dm], bool(center))
    base = torch.randn(C, H, W, generator=gen) * float(want.abs().max())  # (of the size of what is added: acc - base is then exact to rounding)
    gx, acc = c.out("gx", C, H, W), c.inout("gx_acc", base)
    din = c.inp(dm)
    for out, accumulate in ((gx, 0), (acc, 1)):
        c.ok(c.L.maua_gram_flip_bwd(cg.P(din), cg.P(fin), mean_in, kinds, factors, cg.P(out), M, C, H, W, accumulate, c.S()), "maua_gram_flip_bwd")
    c.check("gx", gx, want, TOL)
    c.check("gx accumulated", acc.double().cpu() - base.double(), want, TOL)


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
