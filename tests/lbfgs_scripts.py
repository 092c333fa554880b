"""Scripted gradients for the L-BFGS update (csrc/lbfgs.hip): a fixed list of fp32 gradients that decides, move by move, which curvature
pairs are kept and which are dropped.  Plain torch, no GPU.

The recursion never reads x: lbfgs_pair_kernel forms s = t d from the stored direction and y = g - g_prev, so the list of gradients alone
determines every decision and every move, and the fp64 restatement (oracle.style_oracle._lbfgs_step, one call with max_iter = 1 per
move) can be fed exactly the same list - no objective, no feedback, every single move comparable.

The list is produced by the fp64 restatement alone: before every move but the first, the generator looks at the restatement's last
step s and builds the next gradient so that y.s is what the plan says for that pair.  One plan letter per pair:

  A  accepted: the component of the new gradient along s is g_prev.s_hat + kappa |s|, kappa in 0.7 ... 1.4, so y.s = kappa |s|^2
  N  negative curvature: the same with - kappa |s|
  Z  the gradient repeated: y = 0 and y.s = 0 exactly, on any machine
  T  positive but under the threshold: y.s about 2e-11 (one element j of g_prev moved by 2e-11 / s_j)
  U  just accepted: y.s about 3e-9, built like T.  H_diag = y.s / y.y is then huge and the moves AFTER the one it produces lose
     accuracy (2e-5 ... 1.5e-4 in fp32), so U is the last pair of its script.

For A and N the rest of the new gradient is orthogonal to s: the orthogonal part of g_prev plus 30 % noise, made orthogonal to s again
AFTER the noise went in, and scaled so that |g| = |g_0| where the parallel part leaves room (never below 0.3 |g_0|): the gradients stay
bounded over hundreds of moves.  Where g_prev is parallel to s (always so after a move made with an empty ring: d = -H g) its
"orthogonal part" is rounding residue and not orthogonal to anything; the random direction is used alone.  Wider curvature ranges
diverge (kappa in 0.5 ... 8: 1e12; kappa tied to 1 / |s|: 1e55).

Every gradient is rounded to fp32 before the restatement sees it, so generating and replaying in fp64 are the same computation, and the
records (kind, y.s, |y| |s|) are those of the rounded gradients.
"""
import functools
import math
import random

import torch

from oracle.style_oracle import _LbfgsState, _lbfgs_step

THRESHOLD = 1e-10      # lbfgs.py: `if ys > 1e-10`
T_TARGET = 2e-11
U_TARGET = 3e-9
MOVE_BAR = 2e-4        # the project's bar for a move (tests/test_tuning_variants_gpu.py, tests/test_kernels_gpu.py)
FLOOR = 1e-5           # floor of the ring-wrap test's bar


def _fp32(v):
    return v.float().double()


def _step(st, g, history):
    """One move of the restatement from x = 0 (the recursion does not read x): the move itself."""
    zero = torch.zeros_like(g)
    return _lbfgs_step(zero, lambda v: (0.0, g), st, 1, history)


def _next_gradient(kind, g_prev, s, g0_norm, gen):
    n = g_prev.numel()
    if kind == "Z":
        return g_prev.clone()
    if kind in "TU":
        # j: where |s_j| / |g_j| is largest, so that the fp32 grid of g_j resolves the change; among the elements with a large s_j
        # (after a move with an empty ring s_j / g_j is the same everywhere and a tiny s_j would make |y| |s| large against y.s)
        score = s.abs() / g_prev.abs().clamp_min(1e-30)
        score[s.abs() < 0.5 * s.abs().max()] = -1.0
        j = int(score.argmax())
        g = g_prev.clone()
        g[j] = g[j] + (T_TARGET if kind == "T" else U_TARGET) / s[j]
        return _fp32(g)
    assert kind in "AN", kind
    s_norm = s.norm()
    s_hat = s / s_norm
    kappa = 0.7 + 0.7 * float(torch.rand((), generator=gen, dtype=torch.float64))
    along = g_prev.dot(s_hat)
    par = along + (kappa if kind == "A" else -kappa) * s_norm
    orth = g_prev - along * s_hat
    noise = torch.randn(n, generator=gen, dtype=torch.float64)
    if float(orth.norm()) <= 1e-3 * float(g_prev.norm()):
        orth = noise
    else:
        orth = orth + 0.3 * orth.norm() * noise / noise.norm()
    orth = orth - orth.dot(s_hat) * s_hat
    room = max(g0_norm ** 2 - float(par) ** 2, 0.0)
    orth_norm = max(math.sqrt(room), 0.3 * g0_norm)
    return _fp32(par * s_hat + orth * (orth_norm / orth.norm()))


def make_script(n, history, plan, seed):
    """-> (gradients, records): len(plan) + 1 fp32 gradients as float64 tensors, and per pair (kind, y.s, |y| |s|) of the rounded
    gradients and the fp64 restatement's steps."""
    gen = torch.Generator().manual_seed(seed)
    g0 = _fp32(torch.randn(n, generator=gen, dtype=torch.float64) * 2 / n)   # |g_0|_1 about 1.6: the first step has t < 1
    g0_norm = float(g0.norm())
    st = _LbfgsState()
    gradients, records = [g0], []
    s = _step(st, g0, history)
    for kind in plan:
        g = _next_gradient(kind, gradients[-1], s, g0_norm, gen)
        y = g - gradients[-1]
        records.append((kind, float(y.dot(s)), float(y.norm() * s.norm())))
        gradients.append(g)
        s = _step(st, g, history)
    return gradients, records


def replay(gradients, n, history, dtype):
    """The restatement in `dtype` fed the list: per move x_(k+1) - x_k (float64 tensor), len(st.Y), g.d and t."""
    st = _LbfgsState()
    out = []
    for g in gradients:
        assert g.numel() == n
        gd = g.to(dtype)
        move = _step(st, gd, history)
        out.append(dict(move=move.double(), history_len=len(st.Y), gtd=float(gd.dot(st.d)), t=float(st.t),
                        g_norm=float(g.norm()), d_norm=float(st.d.double().norm())))
    return out


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------------------------
# the plans
# ------------------------------------------------------------------------------------------------------------------------------------
def _plan(pairs, history, seed, p_fill=0.67, p_full=0.67):
    """`NZ` (rejections with an empty ring after the first call), then random letters until the ring is full, then `NANNA` (a rejection
    directly before and after an accepted pair that drops the oldest; a run of two rejections), then random letters: A with
    probability p_fill / p_full, the rest N and Z two to one."""
    rng = random.Random(seed)
    letters, accepted = list("NZ"), 0

    def draw(p):
        u = rng.random()
        return "A" if u < p else ("N" if u < p + (1 - p) * 2 / 3 else "Z")
    while accepted < history and len(letters) < pairs:
        letters.append(draw(p_fill))
        accepted += letters[-1] == "A"
    letters += list("NANNA")
    while len(letters) < pairs:
        letters.append(draw(p_full))
    return "".join(letters[:pairs])


# name -> (n, history, plan, seed).  The seeds of the two long scripts were picked on the CPU among 11 and 16 by the fp32 restatement's
# own worst move against fp64, in the given element order and in three permuted ones (reordered_err32: another summation order of the
# same dot products, which is what another BLAS or the device's sweeps amount to): over ten more orders at most 3.5e-6 and 3.8e-6.
# Other seeds script a badly conditioned sequence of pairs on which fp32 arithmetic itself loses 1e-5 ... 5e-3 and a bar taken from it
# would say little.  A property of the reference alone, asserted in tests/test_lbfgs_scripts_cpu.py.
SCRIPTS = {
    "short-a": (1003, 3, _plan(39, 3, 1), 11),                          # n not a multiple of 4: the scalar sweeps
    "short-b": (1024, 6, _plan(39, 6, 7), 12),
    "multi-wg": (12293, 6, _plan(39, 6, 3), 13),                        # four workgroups of 4096 elements, the last one ragged
    "tri-upper": (1024, 70, _plan(169, 70, 5, p_fill=0.8), 15),
    "eight-reg": (1003, 130, _plan(299, 130, 4, p_fill=0.8), 14),
    "threshold": (1024, 6, "TAATAAU", 17),                              # T with an empty ring, T between accepted pairs, U last
    "short-b-in-70": (1024, 70, _plan(39, 6, 7), 12),                   # short-b's plan in tri-upper's state (the reset tests)
}
# what each script exists for, counted from its records by coverage(): key -> minimum
REQUIRED = {
    "short-a": dict(rejected_empty=2, rejection_runs=1, rejected_full=8, rejected_around_wrap=1),
    "short-b": dict(rejected_empty=2, rejection_runs=1, rejected_full=8, rejected_around_wrap=1),
    "multi-wg": dict(rejected_empty=2, rejection_runs=1, rejected_full=8, rejected_around_wrap=1),
    "tri-upper": dict(rejected_full=15, accepted_full=30),
    "eight-reg": dict(rejected_full=30, accepted_full=50),
    "threshold": dict(t_empty=1, t_between_accepted=1, u_last=1),
    "short-b-in-70": dict(rejected_empty=2, rejection_runs=1),
}
FULL_BEFORE_MOVE = {"tri-upper": 130, "eight-reg": 300}


def coverage(records, history):
    """Counts from the records alone (a pair is accepted when its y.s > 1e-10).  Pair p is decided on move p + 1."""
    acc = [ys > THRESHOLD for _, ys, _ in records]
    kinds = [k for k, _, _ in records]
    length, lens = 0, []           # ring length BEFORE each pair's decision
    for a in acc:
        lens.append(length)
        length = min(history, length + int(a))
    full = [v == history for v in lens]
    c = dict(rejected=acc.count(False), accepted=acc.count(True))
    c["rejected_empty"] = sum(1 for a, v in zip(acc, lens) if not a and v == 0)
    c["rejected_full"] = sum(1 for a, f in zip(acc, full) if not a and f)
    c["accepted_full"] = sum(1 for a, f in zip(acc, full) if a and f)
    c["rejection_runs"] = sum(1 for p in range(1, len(acc)) if not acc[p] and not acc[p - 1] and (p < 2 or acc[p - 2]))
    c["rejected_around_wrap"] = sum(1 for p in range(1, len(acc) - 1) if acc[p] and full[p] and not acc[p - 1] and not acc[p + 1])
    c["first_full_move"] = full.index(True) if True in full else None   # the move after which the ring holds `history` pairs
    c["t_empty"] = sum(1 for k, v in zip(kinds, lens) if k == "T" and v == 0)
    c["t_between_accepted"] = sum(1 for p in range(1, len(acc) - 1) if kinds[p] == "T" and acc[p - 1] and acc[p + 1])
    c["u_last"] = int(bool(kinds) and kinds[-1] == "U" and "U" not in kinds[:-1])
    return c


def reordered_err32(s, seed):
    """The fp32 replay's worst move against fp64 with the elements of every gradient permuted (one permutation for the whole script):
    the same problem, every dot product summed in another order.  None if a ring length differs from the fp64 replay's."""
    perm = torch.randperm(s["n"], generator=torch.Generator().manual_seed(seed))
    r32 = replay([g[perm] for g in s["gradients"]], s["n"], s["history"], torch.float32)
    if [r["history_len"] for r in r32] != [r["history_len"] for r in s["r64"]]:
        return None
    return max(rel_l2(a["move"], b["move"][perm]) for a, b in zip(r32, s["r64"]))


@functools.lru_cache(maxsize=None)
def script(name):
    """Everything the tests need of one script, computed once: the gradients, the records, the fp64 and fp32 replays, the fp32 replay's
    error per move against fp64, and the bar of a move: twice the worst of those plus the floor (the pattern of the ring-wrap test,
    from the restatement alone)."""
    n, history, plan, seed = SCRIPTS[name]
    gradients, records = make_script(n, history, plan, seed)
    r64 = replay(gradients, n, history, torch.float64)
    r32 = replay(gradients, n, history, torch.float32)
    err32 = [rel_l2(a["move"], b["move"]) for a, b in zip(r32, r64)]
    return dict(name=name, n=n, history=history, plan=plan, gradients=gradients, records=records, r64=r64, r32=r32, err32=err32,
                bar=2 * max(err32) + FLOOR)
