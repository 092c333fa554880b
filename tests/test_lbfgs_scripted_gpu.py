"""The L-BFGS update (csrc/lbfgs.hip) driven by scripted gradients (tests/lbfgs_scripts.py), every move and every decision against the fp64
restatement fed the same list.

The keep / drop decision of a curvature pair, the ring's advance and the H_diag in force are taken on the device after every evaluation;
the other L-BFGS tests meet a rejected pair only by chance and allow the ring length a slack of 2.  Here the plan of each script fixes in
advance which pairs are rejected (negative curvature, a repeated gradient, y.s under the 1e-10 threshold), with the ring empty, filling
and full, and tests/test_lbfgs_scripts_cpu.py shows on the restatement alone that no pair is near the threshold: the ring length must be
the restatement's EXACTLY at every move, and a wrong slot, a stale H_diag or a row of M refreshed for a rejected pair shows in the move
it produces.

Driver: x is zeroed before every call, so after it x IS the move (no storage rounding of a large iterate); the device is synchronised
and status() read after every call.  The bar of a move is that of the ring-wrap test (tests/test_tuning_variants_gpu.py): twice the
worst move of the restatement in fp32 arithmetic against fp64 on the same script, plus 1e-5 - from the restatement, never from the device.
Measured numbers: profiles/lbfgs_scripted.md.
"""
import pytest
import torch

import lbfgs_scripts as ls
import plan

pytestmark = pytest.mark.gpu

_FORCED = ("lbfgs_tri", "lbfgs_vec")


@pytest.fixture(scope="module")
def hip():
    import hip as h
    h.lib()
    return h


@pytest.fixture(autouse=True)
def _restore(hip):
    yield
    for k in _FORCED:
        plan.OVERRIDES.pop(k, None)
    plan.forward_to_library(hip.lib())


def force(hip, **fields):
    for k, v in fields.items():
        assert k in _FORCED
        plan.OVERRIDES[k] = str(v)
    plan.forward_to_library(hip.lib())


def device_gradients(s):
    return torch.stack(s["gradients"]).float().cuda()


def run(hip, st, grads, capture=False):
    """The script on state `st`: per move the bits of x (= the move) and status().  capture: ONE iterate reading the static gradient
    buffer is captured into a graph (after an eager warm-up call and a reset, as optim.py does) and replayed for every move."""
    n = grads.shape[1]
    x = torch.zeros(n, device="cuda")
    gbuf = torch.zeros(n, device="cuda")
    graph = None
    if capture:
        gbuf.copy_(grads[0])
        st.iterate(x, gbuf)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st.iterate(x, gbuf)
        st.reset()
    moves, stats = [], []
    for k in range(grads.shape[0]):
        x.zero_()
        gbuf.copy_(grads[k])
        if graph is not None:
            graph.replay()
        else:
            st.iterate(x, gbuf)
        torch.cuda.synchronize()
        stats.append(st.status())
        moves.append(x.clone())
    return torch.stack(moves).cpu(), stats


def against_restatement(hip, name, label):
    s = ls.script(name)
    n, history, r64, bar = s["n"], s["history"], s["r64"], s["bar"]
    assert bar <= ls.MOVE_BAR
    moves, stats = run(hip, hip.LbfgsState(n, history, "cuda"), device_gradients(s))
    worst, worst_gtd = 0.0, 0.0
    for k, (ref, got) in enumerate(zip(r64, stats)):
        e = ls.rel_l2(moves[k], ref["move"])
        e_gtd = abs(got["gtd"] - ref["gtd"]) / (ref["g_norm"] * ref["d_norm"])
        worst, worst_gtd = max(worst, e), max(worst_gtd, e_gtd)
        what = f"{name} [{label}] move {k} (pair {s['plan'][k - 1] if k else '-'})"
        assert got["history_len"] == ref["history_len"], f"{what}: ring length {got['history_len']}, restatement {ref['history_len']}"
        assert got["n_iter"] == k + 1 and not got["stopped"], what
        assert e <= bar, f"{what}: {e:.3e} > {bar:.3e}"
        assert e_gtd <= bar, f"{what}: g.d {got['gtd']:.6e}, restatement {ref['gtd']:.6e}"
        if k == 0:
            assert ref["t"] < 1.0 and abs(got["t"] - ref["t"]) <= 1e-6, what   # min(1, 1 / |g|_1)
        else:
            assert got["t"] == 1.0, what                                          # lr
    print(f"{name} [{label}]: n {n}, history {history}, {len(r64)} moves; fp32 restatement's worst move {max(s['err32']):.3e}, "
          f"bar {bar:.3e}, device's worst move {worst:.3e}, worst |g.d error| / (|g||d|) {worst_gtd:.3e}")


CASES = [
    ("short-a", {}), ("short-a", dict(lbfgs_tri=0)),
    ("short-b", {}), ("short-b", dict(lbfgs_tri=0)), ("short-b", dict(lbfgs_vec=0)),
    ("multi-wg", {}),
    ("tri-upper", {}), ("tri-upper", dict(lbfgs_tri=0)),
    ("eight-reg", {}),
    ("threshold", {}), ("threshold", dict(lbfgs_tri=0)),
    ("short-b-in-70", {}),
]


@pytest.mark.parametrize("name,fields", CASES, ids=[n + "".join(f"-{k}={v}" for k, v in f.items()) for n, f in CASES])
def test_scripted_moves_and_decisions_match_the_restatement(hip, name, fields):
    """short-a (n = 1003: scalar sweeps), short-b (n = 1024: float4 sweeps), multi-wg (four workgroups, the last ragged): rejections
    with an empty ring right after the first call (d = -H_diag g, H_diag still 1), runs of rejections, rejections with the ring full,
    a rejection on either side of an accepted pair that drops the oldest.  tri-upper: lbfgs_coeffs_tri_kernel with 70 pairs, the ring
    full and head advanced by 46: logical pairs 64 ... 69 sit in the second register of a lane and slot_of un-wraps head + i past
    m1 = 71; with lbfgs_tri = 0 the same on lbfgs_coeffs_kernel<4>.  eight-reg: lbfgs_coeffs_kernel<8> (history 130) with 47 rejected
    and 78 accepted pairs while full.  threshold: y.s = 2e-11 (rejected) with an empty ring and between accepted pairs, y.s = 3e-9
    (accepted, H_diag about 1e5) as the last pair."""
    force(hip, **fields)
    against_restatement(hip, name, ", ".join(f"{k}={v}" for k, v in fields.items()) or "default")


def same_run(a, b):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert a[1] == b[1]
    assert not any(st["stopped"] for st in a[1]) and bool(torch.isfinite(a[0]).all())


@pytest.mark.parametrize("name", ["short-b", "tri-upper"])
def test_rerun_leaves_the_same_bits(hip, name):
    s = ls.script(name)
    grads = device_gradients(s)
    same_run(run(hip, hip.LbfgsState(s["n"], s["history"], "cuda"), grads), run(hip, hip.LbfgsState(s["n"], s["history"], "cuda"), grads))


def test_reset_state_behaves_like_a_new_one_bit_for_bit(hip):
    """LbfgsState.reset() (maua_lbfgs_init zeroes the bookkeeping, not the slab), as optim.py calls it when a captured iteration's bundle
    serves the next problem.  (a) a state that ran tri-upper to the end - ring full, head != 0, every slot of the slab and every row of M
    used - and (b) a state whose whole buffer is 0xFF bytes (NaN as floats), each reset and then given short-b's plan: every move and
    every status() equal those of a new state of the same (n, history).  Stale slab contents must not reach a result."""
    big, small = ls.script("tri-upper"), ls.script("short-b-in-70")
    n, history = big["n"], big["history"]
    assert (small["n"], small["history"]) == (n, history)
    grads = device_gradients(small)
    fresh = run(hip, hip.LbfgsState(n, history, "cuda"), grads)

    used = hip.LbfgsState(n, history, "cuda")
    _, stats = run(hip, used, device_gradients(big))
    assert stats[-1]["history_len"] == history and stats[-1]["n_iter"] == len(big["gradients"])
    used.reset()
    same_run(run(hip, used, grads), fresh)

    dirty = hip.LbfgsState(n, history, "cuda")
    torch.cuda.synchronize()
    dirty.buf.fill_(0xFF)
    dirty.reset()
    same_run(run(hip, dirty, grads), fresh)


def test_captured_iterate_replays_the_eager_bits(hip):
    """One iterate captured into a graph (static gradient buffer), then reset and replayed over short-b: every move and every status()
    equal the eager run's, so no decision - keep or drop, the slot, first call or not - is taken on the host at capture time."""
    s = ls.script("short-b")
    grads = device_gradients(s)
    eager = run(hip, hip.LbfgsState(s["n"], s["history"], "cuda"), grads)
    same_run(run(hip, hip.LbfgsState(s["n"], s["history"], "cuda"), grads, capture=True), eager)
    assert [st["history_len"] for st in eager[1]] == [r["history_len"] for r in s["r64"]]
