"""fp64 numpy restatement of the neural cellular automaton (the reference's NCA_train.py / NCA_gen.py) for the tests of
csrc/nca.hip and nca.py.  Written from the reference's behaviour, line numbers cited; no reference code."""
import numpy as np

# the four perception filters as cross-correlation kernels, NCA_train.py:147-149, 161-162 (the /8, /16 comments are not applied)
IDENT = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64)
SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
LAP = np.array([[1, 2, 1], [2, -12, 2], [1, 2, 1]], np.float64)
FILTERS = np.stack([IDENT, SOBEL_X, SOBEL_X.T, LAP])


def perceive(x, filters=FILTERS):
    """NCA_train.py:151-158: every channel under each filter, circular padding 1; output channel 4c + f (channel-major).
    Evaluated in x's own dtype (fp64 for the reference, fp32 for the fp32 twin of the folded-chain test)."""
    b, c, h, w = x.shape
    out = np.zeros((b, c, 4, h, w), x.dtype)
    for f in range(4):
        for i in range(3):
            for j in range(3):
                k = filters[f, i, j]
                if k != 0:
                    out[:, :, f] += x.dtype.type(k) * np.roll(x, shift=(1 - i, 1 - j), axis=(2, 3))
    return out.reshape(b, 4 * c, h, w)


def perceive_t(dp, c, filters=FILTERS):
    """Adjoint of perceive: (b, 4c, h, w) -> (b, c, h, w)."""
    b, _, h, w = dp.shape
    d = dp.reshape(b, c, 4, h, w)
    out = np.zeros((b, c, h, w), dp.dtype)
    for f in range(4):
        for i in range(3):
            for j in range(3):
                k = filters[f, i, j]
                if k != 0:
                    out += dp.dtype.type(k) * np.roll(d[:, :, f], shift=(i - 1, j - 1), axis=(2, 3))
    return out


def split(params, chn, hidden, dtype=np.float64):
    k = 4 * chn
    p = np.asarray(params, dtype)
    return p[:hidden * k].reshape(hidden, k), p[hidden * k:hidden * k + hidden], p[hidden * k + hidden:].reshape(chn, hidden)


def _es(spec, a, b):
    """The contractions go to BLAS (a 300 000-pixel case in seconds); the result in C order, so that what is summed next does not
    depend on the layout BLAS left behind."""
    return np.ascontiguousarray(np.einsum(spec, a, b, optimize=True))


def step(x, params, chn, hidden, mask):
    """CA.forward, NCA_train.py:176-182: x + W2 relu(W1 p + b1) * mask; mask (b, 1, h, w) or (b, h, w).  In x's dtype."""
    w1, b1, w2 = split(params, chn, hidden, x.dtype)
    p = perceive(x)
    a = _es("jk,bkhw->bjhw", w1, p) + b1[None, :, None, None]
    y = _es("cj,bjhw->bchw", w2, np.maximum(a, 0))
    return x + y * mask.reshape(x.shape[0], 1, *x.shape[2:]).astype(x.dtype)


def step_bwd(x, g, params, chn, hidden, mask, relu=None):
    """Analytic backward of step: (dx, dw1, db1, dw2) for dL/dout = g.  relu: a boolean (b, hidden, h, w) array that stands in
    for the decisions a > 0 (h = a where it is set, 0 elsewhere); only the test of the independence claim of near_tie passes it."""
    w1, b1, w2 = split(params, chn, hidden, x.dtype)
    m = mask.reshape(x.shape[0], 1, *x.shape[2:]).astype(x.dtype)
    p = perceive(x)
    a = _es("jk,bkhw->bjhw", w1, p) + b1[None, :, None, None]
    on = (a > 0) if relu is None else relu
    h = np.where(on, a, 0)
    mg = m * g
    dw2 = _es("bchw,bjhw->cj", mg, h)
    da = _es("cj,bchw->bjhw", w2, mg) * on
    dw1 = _es("bjhw,bkhw->jk", da, p)
    db1 = da.sum(axis=(0, 2, 3))
    dp = _es("jk,bjhw->bkhw", w1, da)
    return g + perceive_t(dp, chn), dw1, db1, dw2


def chain_bwd(x0, g_last, params, chn, hidden, masks):
    """BPTT through len(masks) steps: (dx0, flat parameter gradient), in x0's dtype."""
    xs = [x0]
    for m in masks:
        xs.append(step(xs[-1], params, chn, hidden, m))
    g, acc = g_last, np.zeros(len(params), x0.dtype)
    for k in reversed(range(len(masks))):
        g, dw1, db1, dw2 = step_bwd(xs[k], g, params, chn, hidden, masks[k])
        acc += np.concatenate([dw1.ravel(), db1, dw2.ravel()])
    return g, acc


# ---- what the element-wise comparison of one backward step stands on (tests/test_nca_bwd_gpu.py) ----------------------------------
ABS_FILTERS = np.abs(FILTERS)
TIE_TOL = 1e-5


def preact_scale(x, params, chn, hidden):
    """(P, S): P the perception with absolute taps on |x|, S_j = |b1_j| + sum_k |w1_jk| P_k, the sum of the absolute values of
    every term of the pre-activation a_j written out down to the state.  |p| would not do: the Sobel and Laplacian sums cancel,
    and the fp32 error of p (and so of a) scales with the sum of the absolute terms, not with the result."""
    w1, b1, _ = split(params, chn, hidden)
    P = perceive(np.abs(x), ABS_FILTERS)
    return P, _es("jk,bkhw->bjhw", np.abs(w1), P) + np.abs(b1)[None, :, None, None]


def near_tie(x, params, chn, hidden, tol=TIE_TOL):
    """(n, h, w) boolean: pixels where some hidden unit has |a_j| <= tol * S_j, i.e. where an fp32 evaluation may take the ReLU
    decision the other way.  A test zeroes the incoming gradient there: with mask * g = 0, da = 0 whatever the decision, so no
    output of the backward depends on it (proved in tests/test_nca_cpu.py).

    Why tol = 1e-5 covers csrc/nca.hip: the kernel forms p from at most 4 roundings per term (the Laplacian: three additions
    and the final subtraction; 2 * and the pairing are exact or shallower), then a_j = fmaf chain of 4 chn = 48 or 64 terms
    started from b1_j, one rounding per fmaf.  Every term therefore passes through at most 4 chn + 4 <= 68 roundings of at most
    2^-24 relative each: |a32 - a| <= 68 * 2^-24 * S_j = 4.1e-6 S_j < 5e-6 S_j to first order (the second-order terms are 1e-11).
    The fp64 reference's own error is 1e-14 S_j.  tol is twice that bound, so a decision outside the flagged set is the same in
    the kernel and here."""
    w1, b1, _ = split(params, chn, hidden)
    a = _es("jk,bkhw->bjhw", w1, perceive(x)) + b1[None, :, None, None]
    return (np.abs(a) <= tol * preact_scale(x, params, chn, hidden)[1]).any(axis=1)


def step_bwd_abs(x, g, params, chn, hidden, mask, relu=None):
    """The four einsums of step_bwd over absolute values: for every output element the sum of the absolute values of its terms,
    (A_dx, A_dW1, A_db1, A_dW2), written out down to the state (P for p, S for h: see preact_scale).  The ReLU decisions are the
    true ones (or `relu`).  An fp32 evaluation in any fixed order is off by at most (number of roundings a term passes) * 2^-24
    of these."""
    w1, b1, w2 = split(params, chn, hidden)
    m = np.abs(mask.reshape(x.shape[0], 1, *x.shape[2:]))
    a = _es("jk,bkhw->bjhw", w1, perceive(x)) + b1[None, :, None, None]
    on = (a > 0) if relu is None else relu
    P, S = preact_scale(x, params, chn, hidden)
    amg = m * np.abs(g)
    a_dw2 = _es("bchw,bjhw->cj", amg, S * on)
    a_da = _es("cj,bchw->bjhw", np.abs(w2), amg) * on
    a_dw1 = _es("bjhw,bkhw->jk", a_da, P)
    a_db1 = a_da.sum(axis=(0, 2, 3))
    a_dp = _es("jk,bjhw->bkhw", np.abs(w1), a_da)
    return np.abs(g) + perceive_t(a_dp, chn, ABS_FILTERS), a_dw1, a_db1, a_dw2


# ---- the update mask (DESIGN.md "Neural cellular automaton"): floor(u + rate), u a stateless function of (seed, step, b, y, x) --
M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64's output function on uint64 numpy arrays (wrapping arithmetic)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mask_u(seed, step_, n, h, w):
    """u (n, h, w) float32 on the 2^-24 grid."""
    key = mix64(np.uint64(seed & M64) ^ mix64(np.uint64(step_)))
    b = np.arange(n, dtype=np.uint64)[:, None, None]
    y = np.arange(h, dtype=np.uint64)[None, :, None]
    x = np.arange(w, dtype=np.uint64)[None, None, :]
    ctr = (b << np.uint64(40)) | (y << np.uint64(20)) | x
    return (mix64(key ^ ctr) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def mask(seed, step_, n, h, w, rate=0.5, rate_map=None):
    """NCA_train.py:183 `floor(rand + update_rate)` in fp32 with the counter-based u; rate_map (h, w) per pixel (NCA_gen.py:56)."""
    r = np.float32(rate) if rate_map is None else np.asarray(rate_map, np.float32)[None]
    return np.floor(mask_u(seed, step_, n, h, w) + r).astype(np.float32)


# ---- loss and schedules -----------------------------------------------------------------------------------------------------------
def batch_mean_gram_loss(feats, targets):
    """NCA_train.py:134-143 and 235-236: per image einsum(bchw, bdhw -> bcd) / (h w), averaged over the batch, then
    sum over layers of mean((G - T)^2).  feats: list of (b, c, h, w) arrays."""
    total = 0.0
    for f, t in zip(feats, targets):
        b, c, h, w = f.shape
        ff = f.reshape(b, c, h * w).astype(np.float64)
        g = np.einsum("bcn,bdn->bcd", ff, ff) / (h * w)
        total += np.mean((g.mean(0) - t) ** 2)
    return total


def lr(i):
    """Adam(lr 1e-3) with MultiStepLR([2000, 4000], 0.3) stepped after each update (NCA_train.py:207-208, 241)."""
    return 1e-3 * 0.3 ** ((i >= 2000) + (i >= 4000))


def evolution_steps(k):
    return min(2 ** (k // 30), 32)  # NCA_gen.py:17


def rate_map_steps(k):
    return min(int(2 ** (k / 30)), 32)  # NCA_gen.py:55


def seeded(i):
    """x[:1] is reset to the zero seed at every i % 32 == 0 (NCA_train.py:219-220)."""
    return i % 32 == 0


# ---- the single-step backward cases of tests/test_nca_bwd_gpu.py ------------------------------------------------------------------
# Kept here so that tests/test_nca_cpu.py checks, without a GPU, the condition every one of them stands on: near_tie flags at
# most TIE_SHARE of the pixels.  A case added to the GPU file is added here and cannot skip that check.
PAIRS = ((12, 96), (16, 128))
TIE_SHARE = 0.02
BWD_TILE, BWD_MAX_BLOCKS = 64, 1024  # csrc/nca.hip: pixels per tile, partial slots
# pixels: 64 (one full tile), 65, 874 (tile 6 spans two images), 65 536 (1024 tiles: the default training shape, the last that
# does not fold), 65 792 (1028 tiles: slots 0-3 fold once), 102 400 (1600 tiles: slots 0-575 take two), 76 500 (ragged last tile
# while folding), 294 912 (4608 tiles: slots 0-511 take five tiles, the rest four)
PLAN_SHAPES = ((1, 8, 8), (1, 5, 13), (2, 19, 23), (4, 128, 128), (1, 257, 256), (4, 160, 160), (3, 150, 170), (2, 384, 384))
MASK_MODES = ("given", "given_u8", "rate0.5", "rate0.1", "rate_map")
MASK_SHAPES = ((3, 7, 11), (2, 181, 182))  # one small ragged shape (231 pixels), one folded shape (1030 tiles, the last ragged)
ALIAS_PLANES = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 70), (70, 1), (2, 67), (3, 3))
EXTREME_SHAPE = (2, 19, 23)
SLOT_SHAPE = (1, 257, 256)
CHAIN_SHAPE, CHAIN_STEPS = (4, 160, 160), 8


def bwd_cases():
    """(chn, hidden, n, h, w, mode) of every single-step case; mode in MASK_MODES + ("ones", "zeros")."""
    cases = []
    for chn, hidden in PAIRS:
        cases += [(chn, hidden, *s, "rate0.5") for s in PLAN_SHAPES]
        cases += [(chn, hidden, *s, mode) for mode in MASK_MODES for s in MASK_SHAPES]
        cases += [(chn, hidden, n, h, w, "ones" if n == 1 else "rate0.5") for h, w in ALIAS_PLANES for n in (1, 3)]
        cases += [(chn, hidden, *EXTREME_SHAPE, mode) for mode in ("ones", "zeros")]
    return cases


def tiles_per_slot(n, h, w):
    """The most tiles one partial slot of the backward launch takes: ceil(tiles / 1024)."""
    tiles = -(-n * h * w // BWD_TILE)
    return -(-tiles // BWD_MAX_BLOCKS)


def case_params(chn, hidden, seed, w2_scale=0.1, w1_scale=0.2):
    rng = np.random.default_rng(seed)
    k = 4 * chn
    return np.concatenate([rng.normal(0, w1_scale, hidden * k), rng.normal(0, 0.1, hidden),
                           rng.normal(0, w2_scale, chn * hidden)]).astype(np.float32)


# On the smallest planes one flagged pixel is already more than TIE_SHARE (1 of 9 is 11 %), and the circular neighbours alias, so
# Sobel and Laplacian cancel exactly and a sits nearer to zero against its scale: where draw 0 of the state breaks the
# condition, the next draw that keeps it is named here (chosen by near_tie alone, on the CPU, before any kernel ran).
STATE_DRAW = {(12, 1, 5, 13): 1, (12, 3, 1, 1): 1, (12, 1, 2, 1): 1, (12, 1, 3, 3): 1, (16, 3, 70, 1): 1, (16, 3, 3, 3): 1}  # (chn, n, h, w)


def case_state(chn, n, h, w):
    """x ~ N(0, 0.5) and g ~ N(0, 1) in fp32, a function of the pair and the shape alone (so the near-tie map of a shape is the
    same under every mask mode)."""
    rng = np.random.default_rng([chn, n, h, w, STATE_DRAW.get((chn, n, h, w), 0)])
    return rng.normal(0, 0.5, (n, chn, h, w)).astype(np.float32), rng.normal(size=(n, chn, h, w)).astype(np.float32)


def case_mask(n, h, w, mode, seed=11, step_=3):
    """(mask (n, h, w) fp32 as the kernel must see it, keyword arguments that make the kernel produce or read it); an explicit
    mask is passed under "mask" as a numpy array of the dtype the case asks for."""
    rng = np.random.default_rng([n, h, w, 7])
    if mode in ("given", "given_u8"):
        m = (rng.random((n, h, w)) < 0.5).astype(np.float32)
        return m, dict(mask=m.reshape(n, 1, h, w).astype(np.uint8 if mode == "given_u8" else np.float32))
    if mode in ("ones", "zeros"):
        m = np.full((n, h, w), 1.0 if mode == "ones" else 0.0, np.float32)
        return m, dict(mask=m.reshape(n, 1, h, w))
    if mode == "rate_map":
        rmap = rng.random((h, w)).astype(np.float32)
        return mask(seed, step_, n, h, w, rate_map=rmap), dict(rate_map=rmap, seed=seed, step=step_)
    rate = float(mode[4:])
    return mask(seed, step_, n, h, w, rate=rate), dict(rate=rate, seed=seed, step=step_)
