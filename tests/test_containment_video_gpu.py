"""Containment of the img_vid clip kernels (csrc/gauss_wrap.hip): the case of `maua_gauss_wrap` in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the case is registered from here: importing this module appends it to
`test_containment_gpu.TABLE` (its `case` decorator), which is what tests/test_containment_table_cpu.py reads - `pytest tests -m "not gpu"`
imports this module during collection, and the table test then finds `maua_gauss_wrap` covered.  Running
tests/test_containment_table_cpu.py on its own, without this module collected, reports `maua_gauss_wrap` as uncovered.  This module's name
sorts after test_containment_gpu.py, whose `test_contained` is parametrised before this import happens, so every case runs once: the cases
registered here run below, under the same checks as there - the two guard fills (0x00, 0xFF) around everything the entry point reads,
`Ctx.finish()` (guards of everything written intact, every defined element written, the workspace really used), the entry points the
case declares were called, and bit equality of outputs and workspace between the two fills.  Needs neither a GPU nor the library to import.

y sits between 0xA5 guards, x between the run's input guards, the workspace is exactly maua_gauss_wrap_workspace_bytes; the value check is the
bar of tests/test_gauss_wrap_gpu.py: at most twice the distance of scipy's fp32 filter from scipy's float64 one."""
import numpy as np
import pytest
import torch

import test_containment_gpu as cg
from conftest import rel_l2
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)


@cg.case(("maua_gauss_wrap",), [dict(shape=(3, 3, 9, 33), sigmas=(3, 9 / 32, 33 / 32), roll=1), dict(shape=(2, 1, 3, 130), sigmas=(2, 4, 4), roll=0)])
def gauss_wrap_clip(c, shape, sigmas, roll):
    """Three passes (x -> y -> workspace -> y) on planes smaller than a tile and on rows that cross two windows, every axis folded or not."""
    import scipy.ndimage as ndi
    g = torch.Generator().manual_seed(77 + sum(shape))
    x = torch.randn(*shape, generator=g) * 255
    sig = tuple(float(s) for s in sigmas)
    assert c.L.maua_gauss_wrap_supported(*shape, *sig) == 1
    ws = c.used(c.ws("workspace", c.L.maua_gauss_wrap_workspace_bytes(*shape, *sig)))
    y = c.out("y", *shape)
    c.ok(c.L.maua_gauss_wrap(cg.P(c.inp(x)), cg.P(y), *shape, *sig, roll, cg.P(ws), cg.nb(ws), c.S()), "maua_gauss_wrap")
    rolled, sig4 = np.roll(x.numpy(), -roll, axis=0), [sig[0], 0, sig[1], sig[2]]
    ref = ndi.gaussian_filter(rolled.astype(np.float64), sig4, mode="wrap")
    c.check("gauss_wrap", y, ref, 2 * rel_l2(ndi.gaussian_filter(rolled, sig4, mode="wrap"), ref))


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
