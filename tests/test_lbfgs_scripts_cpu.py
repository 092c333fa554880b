"""The scripted gradients of tests/lbfgs_scripts.py are valid scripts: conditions on the fp64 / fp32 restatement alone, so that a failure of
tests/test_lbfgs_scripted_gpu.py cannot be a bad script.  No GPU."""
import math

import pytest
import torch

import lbfgs_scripts as ls

NAMES = sorted(ls.SCRIPTS)


@pytest.mark.parametrize("name", NAMES)
def test_every_decision_is_as_planned(name):
    """A and U are accepted (y.s > 1e-10 exactly), N, Z and T rejected; Z gives y.s = 0 exactly; T and U land where they aim."""
    s = ls.script(name)
    assert len(s["records"]) == len(s["plan"]) == len(s["gradients"]) - 1
    for p, ((kind, ys, _), planned) in enumerate(zip(s["records"], s["plan"])):
        assert kind == planned
        assert (ys > ls.THRESHOLD) == (kind in "AU"), (p, kind, ys)
        if kind == "N":
            assert ys < 0
        if kind == "Z":
            assert ys == 0.0 and torch.equal(s["gradients"][p + 1], s["gradients"][p])
        if kind == "T":
            assert 1.5e-11 <= ys <= 2.5e-11, ys
        if kind == "U":
            assert 2.9e-9 <= ys <= 3.1e-9, ys


@pytest.mark.parametrize("name", NAMES)
def test_ring_lengths_follow_the_records_in_fp64_and_fp32(name):
    """The fp64 replay's ring length is the one the records predict, and the fp32 replay's is the same at every move."""
    s = ls.script(name)
    length, want = 0, [0]
    for _, ys, _ in s["records"]:
        length = min(s["history"], length + int(ys > ls.THRESHOLD))
        want.append(length)
    assert [r["history_len"] for r in s["r64"]] == want
    assert [r["history_len"] for r in s["r32"]] == want


@pytest.mark.parametrize("name", NAMES)
def test_no_pair_is_near_the_threshold(name):
    """|y.s - 1e-10| >= 10 bar |y| |s| for every pair but Z (whose y is zero on any machine): a device whose steps are within the bar of
    the restatement's cannot land on the other side of the threshold.  The bar itself meets the project's bar for a move."""
    s = ls.script(name)
    assert ls.FLOOR <= s["bar"] <= ls.MOVE_BAR, s["bar"]
    ratios = [abs(ys - ls.THRESHOLD) / yn for kind, ys, yn in s["records"] if kind != "Z"]
    print(f"{name}: fp32 restatement's worst move {max(s['err32']):.3e}, bar {s['bar']:.3e}, smallest |y.s - 1e-10| / (|y||s|) {min(ratios):.3e}")
    assert min(ratios) >= 10 * s["bar"]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_arithmetic_in_another_order_stays_under_the_floor(name):
    """The scripts are well conditioned: the restatement in fp32 with every dot product summed in another order (the elements permuted)
    takes the same decisions and its worst move stays under the 1e-5 floor of the bar, as it does in the given order.  A script on
    which fp32 arithmetic loses 1e-4 in one order and 1e-5 in another would make the bar a matter of the host's BLAS."""
    s = ls.script(name)
    errs = [max(s["err32"])] + [ls.reordered_err32(s, seed) for seed in (101, 102)]
    print(f"{name}: fp32 restatement's worst move, given order and two permuted ones: {errs}")
    assert all(e is not None and e <= ls.FLOOR for e in errs)


@pytest.mark.parametrize("name", NAMES)
def test_gradients_and_moves_are_bounded(name):
    """Finite, max-abs in [1e-8, 1e3]; the one move after a U (H_diag about 1e5) is bounded by 1e7.  Every direction descends, the first
    step is shorter than 1 and no move trips the g.d > -tolerance_change = 1 stop: `stopped` stays 0 on the device."""
    s = ls.script(name)
    for k, (g, r) in enumerate(zip(s["gradients"], s["r64"])):
        assert torch.equal(g, g.float().double())      # fp32 values
        assert bool(torch.isfinite(g).all()) and 1e-8 <= float(g.abs().max()) <= 1e3, k
        hi = 1e7 if k > 0 and s["plan"][k - 1] == "U" else 1e3
        assert bool(torch.isfinite(r["move"]).all()) and 1e-8 <= float(r["move"].abs().max()) <= hi, k
        assert r["gtd"] < 0 and math.isfinite(r["gtd"]), k
        assert r["t"] == 1.0 if k else 0.3 < r["t"] < 1.0, k


@pytest.mark.parametrize("name", NAMES)
def test_the_coverage_each_script_exists_for(name):
    s = ls.script(name)
    c = ls.coverage(s["records"], s["history"])
    print(name, c)
    for key, least in ls.REQUIRED[name].items():
        assert c[key] >= least, (key, c[key], least)
    if name in ls.FULL_BEFORE_MOVE:
        assert c["first_full_move"] is not None and c["first_full_move"] < ls.FULL_BEFORE_MOVE[name]
    if name in ("short-a", "short-b", "multi-wg"):
        assert s["plan"].startswith("NZ")
    if "U" in s["plan"]:
        assert s["plan"].index("U") == len(s["plan"]) - 1


def test_shapes_and_kernel_routes():
    """The sizes the table of cases names, and the routes of lbfgs.hip's launcher they stand for."""
    n, h = {k: v[0] for k, v in ls.SCRIPTS.items()}, {k: v[1] for k, v in ls.SCRIPTS.items()}
    assert n["short-a"] % 4 != 0 and n["short-b"] % 4 == 0
    assert math.ceil(n["multi-wg"] / 4096) == 4 and n["multi-wg"] % 4096 not in (0,) and n["multi-wg"] % 4 != 0
    assert 64 < h["tri-upper"] <= 127                   # lbfgs_coeffs_tri_kernel with pairs in both registers of a lane
    assert 2 * (h["eight-reg"] + 1) + 1 > 256           # lbfgs_coeffs_kernel<8>
    assert len(ls.SCRIPTS["threshold"][2]) + 1 <= 9
    assert ls.SCRIPTS["short-b-in-70"][2] == ls.SCRIPTS["short-b"][2] and h["short-b-in-70"] == h["tri-upper"]
    assert n["short-b-in-70"] == n["tri-upper"] == n["short-b"]
    for k, (_, _, plan, _) in ls.SCRIPTS.items():
        assert len(plan) + 1 <= 300
