"""The slab plan of the shifted, mirrored and guided Gram terms (csrc/gram_terms.hpp gt_plan, gt_finish_split) restated in Python and
compared with what the library's host functions answer (no GPU).  The plan - tile pairs, slabs per pair, pixels per slab - is a function
of (C, H W) alone and decides the order in which every matrix element is added, so it decides the bits."""
import pytest

CHANNELS = [1, 3, 64, 65, 70, 130, 450, 512, 513, 65536]
PLANES = [(1, 1), (1, 63), (8, 8), (5, 13), (9, 33), (20, 35), (1024, 1024), (32767, 32767)]
TERMS = [1, 3]
# family -> (all tile pairs?, most slabs per (term, tile pair), most terms per call)
FAMILIES = {"shift": (True, 256, 16), "flip": (False, 768, 4), "guided": (False, 256, 8)}


@pytest.fixture(scope="module")
def L():
    import build_native
    import hip
    build_native.build()
    return hip.lib()


def ceil_div(a, b):
    return -(-a // b)


def pairs(family, c):
    nt = ceil_div(c, 64)
    return nt * nt if FAMILIES[family][0] else nt * (nt + 1) // 2


def plan(family, c, hw):
    """(npairs, ksplit, chunk)"""
    npairs = pairs(family, c)
    stages = ceil_div(hw, 64)
    want = max(1, min(ceil_div(768, npairs), FAMILIES[family][1], stages))
    chunk = ceil_div(ceil_div(hw, want), 64) * 64
    return npairs, ceil_div(hw, chunk), chunk


def expected_bytes(family, terms, c, hw):
    npairs, ksplit, _ = plan(family, c, hw)
    slabs = terms * npairs * ksplit * 16384
    return max(slabs, terms * c * 64 * 8) if family == "guided" else slabs  # guided: the weighted row means' partial sums come first


def workspace_bytes(L, family, terms, c, h, w):
    if family == "guided":
        return L.maua_gram_guided_workspace_bytes(terms, c, h * w)
    return getattr(L, f"maua_gram_{family}_workspace_bytes")(terms, c, h, w)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_workspace_bytes_follow_the_plan(L, family):
    n = 0
    for c in CHANNELS:
        for h, w in PLANES:
            for terms in TERMS:
                assert workspace_bytes(L, family, terms, c, h, w) == expected_bytes(family, terms, c, h * w), (family, terms, c, h, w)
                n += 1
    assert n == 160


def test_plan_restatement_cuts_whole_stages():
    for family in FAMILIES:
        for c in CHANNELS:
            for h, w in PLANES:
                npairs, ksplit, chunk = plan(family, c, h * w)
                assert chunk % 64 == 0 and 1 <= ksplit <= FAMILIES[family][1]
                assert (ksplit - 1) * chunk < h * w <= ksplit * chunk  # every slab has pixels, and together they cover the plane


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_refusals_answer_zero_bytes(L, family):
    most = FAMILIES[family][2]
    assert workspace_bytes(L, family, most, 64, 8, 8) > 0
    for terms, c, h, w in [(0, 64, 8, 8), (most + 1, 64, 8, 8), (1, 65537, 8, 8), (1, 0, 8, 8), (1, 64, 32768, 32768), (1, 64, 1 << 15, 1 << 16)]:
        assert workspace_bytes(L, family, terms, c, h, w) == 0, (family, terms, c, h, w)
    assert workspace_bytes(L, family, 1, 65536, 8, 8) > 0


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_mse_ledger_supported_is_the_record_bound(L, family):
    fn = getattr(L, f"maua_{family}_gram_mse_ledger_supported")
    most = FAMILIES[family][2]
    for c in [64, 450, 512, 1024, 4096, 65536]:
        for terms in (1, most):
            want = any(terms * pairs(family, c) * (16 // fq) <= 4096 for fq in (1, 2, 4))
            assert fn(terms, c) == int(want), (family, terms, c)
    assert fn(0, 64) == 0 and fn(most + 1, 64) == 0 and fn(1, 65537) == 0
