"""CPU / any-device restatement of csrc/flow.hip for tests/test_flow_cpu.py and tests/test_flow_gpu.py (not a test module).

TV-L1 (DESIGN.md "Optical flow") in torch, in the dtype of its inputs (fp64 = the oracle, fp32 = what the same arithmetic loses
in single precision), and the reference's reliability mask (flow.py:77-137) in numpy with the reference's dtypes."""
import math

import numpy as np
import torch

LAMBDA, THETA, TAU, ETA = 0.15, 0.3, 0.25, 0.5


def synth_texture(h, w, seed, dx=0.0, dy=0.0, field=None):
    """(h, w, 3) uint8 RGB texture: a sum of random sinusoids (wavelengths 6-40 px) evaluated at (x - dx, y - dy), or at the points
    `field` = (X, Y) arrays when given."""
    g = np.random.default_rng(seed)
    if field is None:
        y, x = np.mgrid[:h, :w].astype(np.float64)
        X, Y = x - dx, y - dy
    else:
        X, Y = field
    out = np.zeros((h, w, 3))
    for c in range(3):
        acc = np.full((h, w), 127.5)
        for _ in range(12):
            lam, ang, ph = g.uniform(6, 40), g.uniform(0, np.pi), g.uniform(0, 2 * np.pi)
            acc += g.uniform(8, 20) * np.sin(2 * np.pi / lam * (np.cos(ang) * X + np.sin(ang) * Y) + ph)
        out[..., c] = acc
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


# ---- TV-L1 -----------------------------------------------------------------------------------------------------------------
def grey(rgb_u8, dtype=torch.float64):
    t = torch.as_tensor(rgb_u8).to(dtype)
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)  # the kernel's constants are fp32 literals
    return (c(0.299) * t[..., 0] + c(0.587) * t[..., 1]) + c(0.114) * t[..., 2]


def pyr_weights(dtype):
    sigma = 0.6 * math.sqrt(1.0 / (ETA * ETA) - 1.0)
    g = [math.exp(-(t - 3.5) ** 2 / (2 * sigma * sigma)) for t in range(8)]
    s = sum(g)
    return torch.tensor([v / s for v in g], dtype=dtype)


def pyr_down(img):
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    wt = pyr_weights(img.dtype).to(img.device)
    cols = (2 * torch.arange(ow, device=img.device)[:, None] - 3 + torch.arange(8, device=img.device)).clamp(0, w - 1)
    rows = (2 * torch.arange(oh, device=img.device)[:, None] - 3 + torch.arange(8, device=img.device)).clamp(0, h - 1)
    r = (img[:, cols] * wt).sum(-1)               # (h, ow)
    return (r[rows] * wt[None, :, None]).sum(1)   # (oh, ow)


def _grad(I):
    h, w = I.shape
    xi = torch.arange(w, device=I.device)
    yi = torch.arange(h, device=I.device)
    gx = 0.5 * (I[:, (xi + 1).clamp(max=w - 1)] - I[:, (xi - 1).clamp(min=0)])
    gy = 0.5 * (I[(yi + 1).clamp(max=h - 1)] - I[(yi - 1).clamp(min=0)])
    return gx, gy


def warp_prep(i0, i1, u):
    h, w = i0.shape
    y, x = torch.meshgrid(torch.arange(h, device=i0.device, dtype=i0.dtype), torch.arange(w, device=i0.device, dtype=i0.dtype),
                          indexing="ij")
    X = (x + u[0]).clamp(0, w - 1)
    Y = (y + u[1]).clamp(0, h - 1)
    x0 = torch.floor(X).long().clamp(max=max(w - 2, 0))
    y0 = torch.floor(Y).long().clamp(max=max(h - 2, 0))
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    fx, fy = X - x0.to(X.dtype), Y - y0.to(Y.dtype)
    gx, gy = _grad(i1)

    def lerp(P):
        return (1 - fy) * ((1 - fx) * P[y0, x0] + fx * P[y0, x1]) + fy * ((1 - fx) * P[y1, x0] + fx * P[y1, x1])
    iw, wx, wy = lerp(i1), lerp(gx), lerp(gy)
    return torch.stack([wx, wy, ((iw - wx * u[0]) - wy * u[1]) - i0])


def _consts(dtype):
    if dtype == torch.float32:  # the kernel's fp32 constants
        return (torch.tensor(0.15, dtype=torch.float32) * torch.tensor(0.3, dtype=torch.float32),
                torch.tensor(0.3, dtype=torch.float32), torch.tensor(0.25, dtype=torch.float32) / torch.tensor(0.3, dtype=torch.float32))
    return torch.tensor(LAMBDA * THETA, dtype=dtype), torch.tensor(THETA, dtype=dtype), torch.tensor(TAU / THETA, dtype=dtype)


def tv_step(F, S):
    """One TV-L1 iteration: fields F (3, h, w) = [I1wx, I1wy, rho_c], state S (6, h, w) = [u1, u2, p11, p12, p21, p22]."""
    lt, theta, taut = (c.to(S.device) for c in _consts(S.dtype))
    wx, wy, rc = F
    u1, u2, p11, p12, p21, p22 = S
    z = torch.zeros_like(u1)

    def div(px, py):
        a = px.clone()
        a[:, -1] = 0
        b = z.clone()
        b[:, 1:] = px[:, :-1]
        c = py.clone()
        c[-1, :] = 0
        d = z.clone()
        d[1:, :] = py[:-1, :]
        return (a - b) + (c - d)

    g2 = wx * wx + wy * wy
    rho = rc + (wx * u1 + wy * u2)
    f = -rho / torch.where(g2 < 1e-10, torch.ones_like(g2), g2)

    def thresh(u, wc):
        return torch.where(rho < -lt * g2, u + lt * wc,
                           torch.where(rho > lt * g2, u - lt * wc, torch.where(g2 < 1e-10, u, u + f * wc)))
    n1 = thresh(u1, wx) + theta * div(p11, p12)
    n2 = thresh(u2, wy) + theta * div(p21, p22)

    def fgrad(u):
        gx, gy = z.clone(), z.clone()
        gx[:, :-1] = u[:, 1:] - u[:, :-1]
        gy[:-1, :] = u[1:, :] - u[:-1, :]
        return gx, gy
    g1x, g1y = fgrad(n1)
    g2x, g2y = fgrad(n2)
    ng1 = 1 + taut * torch.sqrt(g1x * g1x + g1y * g1y)
    ng2 = 1 + taut * torch.sqrt(g2x * g2x + g2y * g2y)
    return torch.stack([n1, n2, (p11 + taut * g1x) / ng1, (p12 + taut * g1y) / ng1, (p21 + taut * g2x) / ng2, (p22 + taut * g2y) / ng2])


def median5(x):
    """(p, h, w): 5 x 5 median, edge pixels replicated."""
    p, h, w = x.shape
    xp = torch.nn.functional.pad(x[None], (2, 2, 2, 2), mode="replicate")[0]
    win = torch.stack([xp[:, dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)], dim=-1)
    return win.sort(dim=-1).values[..., 12]


def upsample(x, h, w, scale=2.0):
    return torch.nn.functional.interpolate(x[None], size=(h, w), mode="bilinear", align_corners=False)[0] * scale


def levels(h, w, max_levels=5):
    n = 1
    while n < max_levels and (h + 1) // 2 >= 16 and (w + 1) // 2 >= 16:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def estimate(rgb1, rgb2, max_levels=5, warps=5, iters=100, dtype=torch.float64, device="cpu"):
    """The whole coarse-to-fine estimate -> (2, h, w) [u, v]."""
    I0 = [grey(torch.as_tensor(rgb1).to(device), dtype)]
    I1 = [grey(torch.as_tensor(rgb2).to(device), dtype)]
    h, w = I0[0].shape
    for _ in range(1, levels(h, w, max_levels)):
        I0.append(pyr_down(I0[-1]))
        I1.append(pyr_down(I1[-1]))
    S = None
    for l in range(len(I0) - 1, -1, -1):
        H, W = I0[l].shape
        new = torch.zeros(6, H, W, dtype=dtype, device=device)
        if S is not None:
            new[:2] = upsample(S[:2], H, W, 1.0 / ETA)
        S = new
        for _ in range(warps):
            F = warp_prep(I0[l], I1[l], S[:2])
            for _ in range(iters):
                S = tv_step(F, S)
            S = torch.cat([median5(S[:2]), S[2:]])
    return S[:2]


# ---- reliability mask (reference flow.py:77-137), numpy with the reference's dtypes ---------------------------------------------
def classify(flow1, flow2):
    """1 reliable, -1 round trip inconsistent, 0 outside the frame or motion edge: the field the reference blurs."""
    f1 = np.asarray(flow1, np.float32)
    f2 = np.asarray(flow2, np.float32)
    h, w = f1.shape[:2]
    y, x = np.mgrid[:h, :w]
    v1, u1 = f1[..., 1], f1[..., 0]
    wy, wx = y + v1.astype(np.float64), x + u1.astype(np.float64)
    cy, cx = np.clip(wy, 0, h - 2), np.clip(wx, 0, w - 2)
    iy, ix = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
    a0, a1 = cy - iy, cx - ix
    wc = []
    for c in (1, 0):  # v, then u
        g = f2[..., c].astype(np.float64)
        b0 = (1 - a1) * g[iy, ix] + a1 * g[iy, ix + 1]
        b1 = (1 - a1) * g[iy + 1, ix] + a1 * g[iy + 1, ix + 1]
        wc.append((1 - a0) * b0 + a0 * b1)
    dy, dx = (wy + wc[0]) - y, (wx + wc[1]) - x
    sq = dy * dy + dx * dx
    thr = 0.01 * ((wc[0] * wc[0] + (v1 * v1).astype(np.float64)) + (wc[1] * wc[1] + (u1 * u1).astype(np.float64))) + 0.5
    r = np.where(sq >= thr, -1, 1)
    r = np.where((wy < 0) | (wx < 0) | (wy >= h - 1) | (wx >= w - 1), 0, r)
    me = np.zeros((h, w))
    for c in (1, 0):
        g = f1[..., c].astype(np.float64)
        ddx = np.concatenate([g[:, 1:], np.zeros((h, 1))], axis=1) - g
        ddy = np.concatenate([g[1:], np.zeros((1, w))], axis=0) - g
        me = me + (ddx * ddx + ddy * ddy) if c == 0 else (ddx * ddx + ddy * ddy)
    mt = np.float32(0.01) * (v1 * v1 + u1 * u1) + np.float32(0.002)
    return np.where((me > mt.astype(np.float64)) & (r != -1), 0, r).astype(np.int8)


def erode41(cls):
    """1 where the 41 x 41 window (clamped to the frame) is all 1, else 0."""
    ok = (np.asarray(cls) == 1)
    h, w = ok.shape
    col = np.stack([ok[max(0, y - 20):y + 21].all(axis=0) for y in range(h)])
    return np.stack([col[:, max(0, x - 20):x + 21].all(axis=1) for x in range(w)], axis=1).astype(np.int64)


def mask_bytes(flow1, flow2):
    return ((1 - erode41(classify(flow1, flow2))) * 255).astype(np.uint8)


def fixture_cases(path):
    """tests/golden/flow_consistency.npz (tools/make_flow_golden.py) as a list of dicts: kind, flow1 / flow2 ((h, w, 2) float32,
    rebuilt exactly from the stored int16 row differences and power-of-two steps), class (the reference's field before its blur),
    mask (the PNG bytes it saves) and color (its flow_to_image of flow1)."""
    g = np.load(path)
    out = []
    for i, kind in enumerate(str(k) for k in g["kinds"]):
        s1, s2 = (int(v) for v in g[f"shift_{i}"])
        flows = [(np.cumsum(g[f"q{j}_{i}"], axis=1, dtype=np.int16).astype(np.float64) * 2.0 ** -s).astype(np.float32)
                 for j, s in ((1, s1), (2, s2))]
        out.append(dict(kind=kind, flow1=flows[0], flow2=flows[1], cls=g[f"class_{i}"], mask=g[f"mask_{i}"], color=g[f"color_{i}"]))
    return out
