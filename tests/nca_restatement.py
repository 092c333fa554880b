"""fp64 numpy restatement of the neural cellular automaton (the reference's NCA_train.py / NCA_gen.py) for the tests of
csrc/nca.hip and nca.py.  Written from the reference's behaviour, line numbers cited; no reference code."""
import numpy as np

# the four perception filters as cross-correlation kernels, NCA_train.py:147-149, 161-162 (the /8, /16 comments are not applied)
IDENT = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64)
SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
LAP = np.array([[1, 2, 1], [2, -12, 2], [1, 2, 1]], np.float64)
FILTERS = np.stack([IDENT, SOBEL_X, SOBEL_X.T, LAP])


def perceive(x):
    """NCA_train.py:151-158: every channel under each filter, circular padding 1; output channel 4c + f (channel-major)."""
    b, c, h, w = x.shape
    out = np.zeros((b, c, 4, h, w), np.float64)
    for f in range(4):
        for i in range(3):
            for j in range(3):
                k = FILTERS[f, i, j]
                if k != 0:
                    out[:, :, f] += k * np.roll(x, shift=(1 - i, 1 - j), axis=(2, 3))
    return out.reshape(b, 4 * c, h, w)


def perceive_t(dp, c):
    """Adjoint of perceive: (b, 4c, h, w) -> (b, c, h, w)."""
    b, _, h, w = dp.shape
    d = dp.reshape(b, c, 4, h, w)
    out = np.zeros((b, c, h, w), np.float64)
    for f in range(4):
        for i in range(3):
            for j in range(3):
                k = FILTERS[f, i, j]
                if k != 0:
                    out += k * np.roll(d[:, :, f], shift=(i - 1, j - 1), axis=(2, 3))
    return out


def split(params, chn, hidden):
    k = 4 * chn
    p = np.asarray(params, np.float64)
    return p[:hidden * k].reshape(hidden, k), p[hidden * k:hidden * k + hidden], p[hidden * k + hidden:].reshape(chn, hidden)


def step(x, params, chn, hidden, mask):
    """CA.forward, NCA_train.py:176-182: x + W2 relu(W1 p + b1) * mask; mask (b, 1, h, w) or (b, h, w)."""
    w1, b1, w2 = split(params, chn, hidden)
    p = perceive(x)
    a = np.einsum("jk,bkhw->bjhw", w1, p) + b1[None, :, None, None]
    y = np.einsum("cj,bjhw->bchw", w2, np.maximum(a, 0))
    return x + y * mask.reshape(x.shape[0], 1, *x.shape[2:])


def step_bwd(x, g, params, chn, hidden, mask):
    """Analytic backward of step: (dx, dw1, db1, dw2) for dL/dout = g."""
    w1, b1, w2 = split(params, chn, hidden)
    m = mask.reshape(x.shape[0], 1, *x.shape[2:])
    p = perceive(x)
    a = np.einsum("jk,bkhw->bjhw", w1, p) + b1[None, :, None, None]
    h = np.maximum(a, 0)
    mg = m * g
    dw2 = np.einsum("bchw,bjhw->cj", mg, h)
    da = np.einsum("cj,bchw->bjhw", w2, mg) * (a > 0)
    dw1 = np.einsum("bjhw,bkhw->jk", da, p)
    db1 = da.sum(axis=(0, 2, 3))
    dp = np.einsum("jk,bjhw->bkhw", w1, da)
    return g + perceive_t(dp, chn), dw1, db1, dw2


def chain_bwd(x0, g_last, params, chn, hidden, masks):
    """BPTT through len(masks) steps: (dx0, flat parameter gradient)."""
    xs = [x0]
    for m in masks:
        xs.append(step(xs[-1], params, chn, hidden, m))
    g, acc = g_last, np.zeros(len(params))
    for k in reversed(range(len(masks))):
        g, dw1, db1, dw2 = step_bwd(xs[k], g, params, chn, hidden, masks[k])
        acc += np.concatenate([dw1.ravel(), db1, dw2.ravel()])
    return g, acc


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
