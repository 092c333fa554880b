"""The engine's decisions - which ReLU inputs it took as positive, which element of every max-pooling window it took as the maximum -
read from an evaluated StyleEngine and laid out as the `decisions` of oracle.OracleNet.feval (spec index -> bool mask for a relu,
int64 flat indices shaped like the pooled map for a max pool, the layout of F.max_pool2d(return_indices=True)).

An oracle pinned to these decisions differs from the engine by arithmetic alone: near a tie no fp32 implementation can take fp64's
decisions, and one decision taken the other way moves the pixel gradient by 1e-3, a thousand times the arithmetic.

Engine steps are matched to spec entries in order: a conv step with a fused ReLU is one conv entry plus one relu entry; every relu and
every max pool of the spec gets exactly one decision source:
- a materialised post-ReLU activation: the mask is `act > 0`;
- a 2x2 / 2 max pool with decision bytes (engine.pool_codes, one byte per window, planar layout by conftest.planar_codes): the arg-max is
  the corner in bits 1:0 (2 dy + dx).  Where the convolution's epilogue pooled and the activation itself was never written (a meta
  tensor), bit 2 says the ReLU input at the arg-max was not positive; the rest of such a window passes no gradient and feeds nothing
  else, so its mask is the reference forward's own;
- any other max pool (odd planes, NIN's 3 x 3 / 2 ceil-mode pools): F.max_pool2d on the engine's own pooled-from activation.  The kernels
  use ATen's tie rule - first maximum in row-major order, NaN wins (csrc/pointwise.hip, window_argmax) - so ATen's indices on the
  engine's values ARE the engine's decisions."""
import torch
import torch.nn.functional as F

from conftest import planar_codes

# The number of decisions the engine takes differently from fp64 may exceed the fp32 oracle's count on the same inputs by this factor plus
# a constant (set from the counts measured on the committed cases, profiles/pinned_parity.md, with 2x headroom): more flips than that
# would mean the engine's arithmetic is further from fp64 near the ReLU and pooling boundaries than fp32 arithmetic is.
FLIP_FACTOR, FLIP_SLACK = 2, 4


def step_map(engine, spec):
    """{spec index: engine step} for every conv, relu and pool entry of `spec`, in order (a fused conv + ReLU step serves both)."""
    entries = [i for i, l in enumerate(spec) if l.kind in ("conv", "relu", "pool")]
    out, j = {}, 0

    def take(kind, s):
        nonlocal j
        assert j < len(entries), ("engine has more layers than the spec", kind)
        i = entries[j]
        assert spec[i].kind == kind, (i, spec[i].kind, kind)
        out[i] = s
        j += 1
        return i

    for s in engine.steps:
        if s.kind == "conv":
            i = take("conv", s)
            l = spec[i]
            assert (l.k, l.stride, l.pad, l.cout, l.cin) == (s.k, s.stride, s.pad, s.mod.out_channels, s.mod.in_channels), (i, l.name)
            if s.relu:
                take("relu", s)
        elif s.kind == "relu":
            take("relu", s)
        elif s.kind == "pool":
            i = take("pool", s)
            l = spec[i]
            assert (l.k, l.stride, l.ceil, l.pool_mode) == (s.k, s.stride, s.ceil, s.mode), (i, s.k, s.stride, s.ceil, s.mode)
    assert j == len(entries), ("spec has layers the engine does not run", entries[j:])
    return out


def activation_map(engine, spec):
    """{engine activation index: spec index of the same tensor}: a conv's output (ReLU'd in the launch or in place) is the relu entry's
    activation, a pool's output the pool entry's."""
    out = {}
    for i, s in step_map(engine, spec).items():
        if spec[i].kind in ("relu", "pool"):
            assert s.dst not in out or spec[out[s.dst]].kind == "relu", (i, s.dst)
            out[s.dst] = i
    return out


def _code_indices(codes, w_in):
    """Flat input indices of the arg-max corners in planar decision bytes (n, c, h / 2, w / 2)."""
    codes = codes.long()
    hp, wp = codes.shape[2:]
    py = torch.arange(hp).view(1, 1, hp, 1)
    px = torch.arange(wp).view(1, 1, 1, wp)
    return (2 * py + ((codes & 3) >> 1)) * w_in + 2 * px + (codes & 1)


def oracle_decisions(spec, acts, aux):
    """An oracle forward's own decisions (OracleNet._forward's acts and aux), in the `decisions` layout."""
    out = {}
    for i, l in enumerate(spec):
        if l.kind == "relu":
            out[i] = acts[i] > 0
        elif l.kind == "pool" and l.pool_mode == "max":
            out[i] = aux[i]
    return out


def count_flips(spec, decisions, acts, aux):
    """{spec index: decisions taken differently from the oracle forward (acts, aux)}: ReLU masks that differ; max-pool arg-maxes that
    differ where that forward's window maximum is positive (a maximum of zero passes no gradient)."""
    out = {}
    for i, d in decisions.items():
        if spec[i].kind == "relu":
            out[i] = int((d ^ (acts[i] > 0)).sum())
        else:
            out[i] = int(((d != aux[i]) & (acts[i] > 0)).sum())
    return out


def engine_decisions(engine, spec, acts, aux):
    """(decisions, flips) of an evaluated engine (B = 1): `decisions` for OracleNet.feval, `flips` = count_flips against the oracle
    forward (acts, aux) - the unpinned forward of the oracle the decisions will pin, which also fills in the masks the engine never
    materialised (see the module docstring)."""
    steps = step_map(engine, spec)
    act = engine.act
    out = {}
    for i, s in steps.items():
        l = spec[i]
        if l.kind == "pool" and l.pool_mode == "max":
            src = act[s.src]
            assert src is None or src.shape[0] == 1, "B = 1 only"
            if id(s) in engine.pool_codes:
                out[i] = _code_indices(planar_codes(engine.pool_codes[id(s)].cpu()), acts[i - 1].shape[3])
            else:
                assert src is not None and not src.is_meta, (i, "a max pool without decision bytes needs its input")
                out[i] = F.max_pool2d(src.cpu(), l.k, l.stride, 0, ceil_mode=l.ceil, return_indices=True)[1]
    for i, s in steps.items():
        if spec[i].kind != "relu":
            continue
        a = act[s.dst]
        assert a.shape[0] == 1, "B = 1 only"
        if not a.is_meta:
            out[i] = a.cpu() > 0
            continue
        pool = engine.fused_pool[id(s)]   # (the only reason an activation is a shape only: its pool ran in the conv's epilogue)
        j = next(k for k, t in steps.items() if t is pool)
        assert j == i + 1 or all(spec[k].kind in ("content", "style") for k in range(i + 1, j)), (i, j)
        codes = planar_codes(engine.pool_codes[id(pool)].cpu())
        mask = (acts[i] > 0).clone()
        flat = mask.reshape(*mask.shape[:2], -1)
        flat.scatter_(2, out[j].reshape(*out[j].shape[:2], -1), (codes & 4).reshape(*codes.shape[:2], -1) == 0)
        out[i] = mask
    assert set(out) == {i for i, l in enumerate(spec) if l.kind == "relu" or (l.kind == "pool" and l.pool_mode == "max")}
    return out, count_flips(spec, out, acts, aux)
