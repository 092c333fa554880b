"""Containment of the guided Gram entry points (csrc/gram_guided.hip): their cases in the table of tests/test_containment_gpu.py.

That module is a yardstick and stays as it is, so the cases are registered from here, as tests/test_containment_video_gpu.py does: importing
this module appends them to `test_containment_gpu.TABLE`, which tests/test_containment_table_cpu.py reads during a collection of the whole
suite; this module's name sorts after test_containment_gpu.py, so every case runs once, below, under the same checks - the two guard
fills (0x00, 0xFF) around everything an entry point reads, `Ctx.finish()` (guards of everything written intact, every defined element
written, the workspace really used), the declared entry points called, and bit equality of outputs and workspace between the fills.

Shapes: channels that are no multiple of the 64-channel tile (two tile pairs and a ragged one), planes that end inside a 64-pixel stage and
inside the backward kernel's 256-pixel tile, one plane smaller than a stage; three regions - a hard mask, a soft one, and one without mass
(inactive: its matrix and means must be WRITTEN as zeros).  The workspace is exactly maua_gram_guided_workspace_bytes.  Value bar: TOL of
tests/test_kernels_gpu.py for contractions (2e-5), as in tests/test_gram_guided_gpu.py."""
import pytest
import torch

import test_containment_gpu as cg
from test_containment_gpu import _restore, recorded  # noqa: F401  (fixtures: the recording proxy, and the library state put back)

pytestmark = pytest.mark.gpu

FIRST = len(cg.TABLE)
TOL = 2e-5
SHAPES = [dict(C=70, N=297, center=1), dict(C=70, N=297, center=0), dict(C=3, N=5, center=1), dict(C=130, N=700, center=1)]


def _inputs(C, N):
    g = torch.Generator().manual_seed(31 + C + N)
    f = torch.relu(torch.randn(C, N, generator=g) + 0.3)
    guides = torch.zeros(3, N)
    guides[0, N // 3:] = 1                       # hard: zero over the first third
    guides[1] = torch.rand(N, generator=g)       # soft
    guides[2, 0] = 0.5                           # mass 0.25: inactive
    return f, guides, g


def _reference(f, guides, center):
    f64, g64 = f.double(), guides.double()
    C = f.shape[0]
    mass = (g64 * g64).sum(1)
    grams, means, scale = [], [], []
    for r in range(guides.shape[0]):
        act = bool(mass[r] >= 1.0)
        mu = (f64 * (g64[r] ** 2)[None]).sum(1) / mass[r] if (center and act) else torch.zeros(C, dtype=torch.float64)
        x = (f64 - mu[:, None]) * g64[r][None]
        scale.append(1.0 / (C * float(mass[r])) if act else 0.0)
        grams.append(x @ x.t() * scale[-1])
        means.append(mu)
    return mass, torch.tensor(scale, dtype=torch.float64), torch.stack(grams), torch.stack(means)


@cg.case(("maua_gram_guided_mass", "maua_gram_guided_fwd", "maua_gram_guided_bwd"), SHAPES)
def gram_guided(c, C, N, center):
    f, guides, gen = _inputs(C, N)
    R = guides.shape[0]
    mass64, scale64, gram64, mean64 = _reference(f, guides, center)
    assert c.L.maua_gram_guided_supported(R, C, N) == 1
    # mass
    mass = c.out("mass", R, dtype=torch.float64)
    c.ok(c.L.maua_gram_guided_mass(cg.P(c.inp(guides)), cg.P(mass), R, N, c.S()), "maua_gram_guided_mass")
    c.check("mass", mass, mass64, 1e-12)
    # forward
    scale = scale64.float()
    ws = c.used(c.ws("workspace", c.L.maua_gram_guided_workspace_bytes(R, C, N)))
    gram = c.out("gram", R, C, C)
    mean = c.out("mean", R, C) if center else None
    c.ok(c.L.maua_gram_guided_fwd(cg.P(c.inp(f)), cg.P(c.inp(guides)), cg.P(c.inp(scale)), cg.P(c.inp(mass64)) if center else None, cg.P(gram),
                                  cg.P(mean), R, C, N, center, cg.P(ws), cg.nb(ws), c.S()), "maua_gram_guided_fwd")
    torch.cuda.synchronize()
    for r in range(R):
        assert torch.equal(gram[r], gram[r].t())
        if scale64[r] == 0:
            assert not bool(gram[r].any()) and (mean is None or not bool(mean[r].any()))
        else:
            c.check(f"gram[{r}]", gram[r], gram64[r], TOL)
    # backward, both accumulate forms; the means are read from a copy between input guards
    d = torch.randn(R, C, C, generator=gen)
    d = d + d.transpose(1, 2)
    want = sum(float(scale64[r]) * (d[r].double() @ (f.double() - mean64[r][:, None])) * (guides[r].double() ** 2)[None] for r in range(R))
    base = torch.randn(C, N, generator=gen) * float(want.abs().max())  # (of the size of what is added: acc - base is then exact to rounding)
    mean_in = cg.P(c.inp(mean64.float())) if center else None
    gf, acc = c.out("gf", C, N), c.inout("gf_acc", base)
    for out, accumulate in ((gf, 0), (acc, 1)):
        c.ok(c.L.maua_gram_guided_bwd(cg.P(c.inp(d)), cg.P(c.inp(f)), cg.P(c.inp(guides)), cg.P(c.inp(scale)), mean_in, cg.P(out), R, C, N,
                                      accumulate, c.S()), "maua_gram_guided_bwd")
    c.check("gf", gf, want, TOL)
    c.check("gf accumulated", acc.double().cpu() - base.double(), want, TOL)


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
