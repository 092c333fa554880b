"""csrc/gauss_wrap.hip through hip.gauss_wrap against scipy: the periodic Gaussian over time and space of the img_vid clip path.

"theirs" is scipy.ndimage.gaussian_filter(mode="wrap") on the fp32 array - the code the host path of style.img_vid runs; the reference is
the same call on the float64 array.  Both distances are measured here and printed; the bar is rel_l2(ours, ref) <= 2 * rel_l2(theirs, ref)
with no absolute floor (a kernel that sums in fp64 and rounds once per filtered axis sits at the distance of theirs).

CASES are seven seeded shapes of the clip path (one frame, both `--init` proportions, the between-scale blend, axes shorter than the
radius, odd extents, the real clip length).  PATHS adds the smallest shapes at which the launch code takes its other routes (csrc/gauss_wrap.hip:
gw_tile, gw_launch): a strided pass that stages its whole axis in more than 64 KiB of LDS, one in windows cut down to the LDS cap, one in
plain windows, strided passes whose tile does not fit LDS at all (taps from global memory), plain and folded, a row pass with several
windows per row, and H or W as the first pass of a rolled clip."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

CASES = [
    ((1, 3, 5, 7), (1, 5 / 32, 7 / 32)),       # one frame, every tap the same element
    ((3, 3, 9, 33), (3, 9 / 32, 33 / 32)),     # --init random proportions, tiny
    ((5, 3, 40, 70), (5, 4, 4)),               # --init content
    ((9, 3, 33, 65), (0.5, 0, 0)),             # the between-scale blend, five taps, no fold
    ((2, 1, 3, 130), (2, 4, 4)),               # H shorter than the radius; W crosses a 128 tile
    ((7, 3, 16, 16), (7, 0.5, 0.5)),           # odd extents, fold on T only
    ((48, 3, 64, 96), (48, 2, 3)),             # the real clip length, 385 taps folded onto 48
]
PATHS = [
    ((1, 2, 600, 3), (0, 70, 0)),              # 561 taps on 600 rows: the whole column staged (150 KiB of LDS)
    ((1, 1, 700, 3), (0, 70, 0)),              # 561 taps on 700 rows: windows of 48 rows, as many as the LDS cap leaves beside the halo
    ((3, 1, 700, 5), (0, 80, 0)),              # 641 taps on 700 rows: no tile fits, taps from global memory; H is the first pass
    ((1, 1, 650, 3), (0, 100, 0)),             # 801 taps folded onto 650 rows: the same, folded
    ((2, 1, 150, 70), (0, 2, 0)),              # 17 taps on 150 rows: three windows of 64 rows (the last one short), two column tiles
    ((2, 1, 2, 1100), (0, 0, 4)),              # 33 taps on rows of 1100: two windows per row; W is the first pass
    ((9, 2, 70, 3), (0, 2, 0.1)),              # H staged whole, then a one-tap W pass
]
ROLLS = (0, 7, -3)


@functools.lru_cache(maxsize=None)
def case(shape, sigmas, roll):
    """x = randn * 255 (seeded), theirs (fp32 scipy) and the fp64 reference for one roll; computed once, never written."""
    import scipy.ndimage as ndi
    g = torch.Generator().manual_seed(1000 + sum(shape) + 7 * len(shape))
    x = (torch.randn(*shape, generator=g) * 255).numpy()
    sig = [sigmas[0], 0, sigmas[1], sigmas[2]]
    rolled = np.roll(x, -roll, axis=0)
    theirs = ndi.gaussian_filter(rolled, sig, mode="wrap")
    ref = ndi.gaussian_filter(rolled.astype(np.float64), sig, mode="wrap")
    for a in (x, theirs, ref):
        a.setflags(write=False)
    return x, theirs, ref


def ours_of(x, sigmas, roll, **kw):
    import hip
    return hip.gauss_wrap(torch.from_numpy(np.array(x)).cuda(), sigmas, roll=roll, **kw)


@pytest.mark.parametrize("roll", ROLLS)
@pytest.mark.parametrize("shape, sigmas", CASES + PATHS, ids=lambda v: "x".join(f"{s:g}" for s in v))
def test_against_scipy(shape, sigmas, roll):
    x, theirs, ref = case(shape, sigmas, roll)
    ours = ours_of(x, sigmas, roll)
    assert ours.shape == tuple(shape) and ours.dtype == torch.float32 and ours.is_cuda
    ours = ours.cpu()
    e_ours, e_theirs = rel_l2(ours, ref), rel_l2(theirs, ref)
    print(f"gauss_wrap {shape} {sigmas} roll {roll}: ours {e_ours:.3e}  theirs {e_theirs:.3e}  ours vs theirs {rel_l2(ours, theirs):.3e}")
    assert torch.isfinite(ours).all()
    assert e_ours <= 2 * e_theirs, (shape, sigmas, roll, e_ours, e_theirs)


@pytest.mark.parametrize("roll", (0, 1, 7, -3, 100))
def test_no_filtered_axis_is_the_rolled_clip_bit_for_bit(roll):
    import hip
    x = torch.from_numpy(np.array(case((9, 3, 33, 65), (0.5, 0, 0), 0)[0])).cuda()
    assert hip.lib().maua_gauss_wrap_workspace_bytes(9, 3, 33, 65, 0.0, 0.0, 0.0) == 0
    ours = hip.gauss_wrap(x, (0, 0, 0), roll=roll)
    assert torch.equal(ours, torch.roll(x, -roll, 0))


def test_reruns_are_bit_identical():
    shape, sigmas = CASES[2]
    x = case(shape, sigmas, 7)[0]
    first = ours_of(x, sigmas, 7)
    for _ in range(3):
        assert torch.equal(ours_of(x, sigmas, 7), first)


@pytest.mark.parametrize("shape, sigmas", [CASES[1], CASES[3], CASES[4]], ids=lambda v: "x".join(f"{s:g}" for s in v))
def test_caller_workspace_of_exactly_workspace_bytes(shape, sigmas):
    import hip
    need = hip.lib().maua_gauss_wrap_workspace_bytes(*shape, *(float(s) for s in sigmas))
    tables = sum(-(-min(2 * int(4.0 * s + 0.5) + 1, ext) * 8 // 256) * 256 for s, ext in zip(sigmas, (shape[0], shape[2], shape[3])) if s > 1e-15)
    passes = sum(s > 1e-15 for s in sigmas)
    assert need == tables + (4 * int(np.prod(shape)) if passes >= 2 else 0)
    x = case(shape, sigmas, 1)[0]
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.equal(ours_of(x, sigmas, 1, workspace=ws), ours_of(x, sigmas, 1))


def test_refusals_raise_before_any_launch():
    import hip
    shape, sigmas = CASES[1]
    x = torch.from_numpy(np.array(case(shape, sigmas, 0)[0])).cuda()
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(x.cpu(), sigmas)
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(x[0], sigmas)
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(x, (3, -1.0, 1))
    with pytest.raises(hip.HipError):
        hip.gauss_wrap(x, (float("nan"), 1, 1))
    before = x.clone()
    with pytest.raises(hip.HipError, match="same buffer"):
        hip.gauss_wrap(x, sigmas, out=x)
    need = hip.lib().maua_gauss_wrap_workspace_bytes(*shape, *(float(s) for s in sigmas))
    short = torch.full((need - 1,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full_like(x, float("nan"))
    with pytest.raises(hip.HipError, match="workspace too small"):
        hip.gauss_wrap(x, sigmas, workspace=short, out=out)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((short == 0xFF).all()) and bool(torch.isnan(out).all())  # nothing was launched
