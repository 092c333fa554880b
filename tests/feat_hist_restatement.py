"""Restatement of the feature-histogram style loss (Risser, Wilmot & Barnes 2017) on the CPU: the decisions in numpy float32 exactly as
DESIGN.md section 15 writes them, everything else in fp64.

For one frame F (C, H, W) of a style layer (N = H W), a target table T (C, K) (non-decreasing along k) and NB bins, per channel c:
  range      lo = min F[c], hi = max F[c], of F rounded to float32 (exact for a float32 input);
  bin        inv = float32(float64(NB) / (float64(hi) - float64(lo))), 0 where hi == lo;  t = fl32(fl32(v - lo) * inv) - one float32
             subtraction, one float32 multiplication;  b = min(NB - 1, int(t));  frac = min(1, fl32(t - float32(b)));
  counts     cnt[b] integers, cum their exclusive prefix sum, cum[NB] = N;
  match      q = (cum[b] + frac cnt[b]) / N;  p = clamp(q K - 0.5, 0, K - 1);  i0 = min(K - 2, floor(p));
             R = T[c][i0] + (p - i0) (T[c][i0 + 1] - T[c][i0])                                  (fp64)
  term       h = mean over c, i of (F - R)^2, R a constant in the derivative: dh/dF = 2 (F - R) / (C N).
  table      of a style activation S (C, Hs, Ws), N_s = Hs Ws: T[c][k] = sorted(S[c])[min(N_s - 1, floor((k + 0.5) N_s / K))]; several style
             images add blend weight x T.
  loss       t' = t + [shift terms] + [mirror terms] + hist_loss_factor h, t the static scalar; the static term is acc(t') s and the dynamic
             one (video_style_factor > 0) stays vsf acc(t) s.
The network around the style layers is oracle.style_oracle's (by way of tests/flip_restatement.py), differentiated by autograd.
"""
import numpy as np
import torch

import flip_restatement as fr
import shift_restatement as sr
from guided_restatement import _ScaleGradients
from oracle.style_oracle import adam_run, lbfgs_run, loss_order  # noqa: F401

BINS, KNOTS = 256, 1024  # the defaults of the preset keys hist_loss_bins / hist_loss_knots


def quantile_index(n, knots):
    """min(n - 1, floor((k + 0.5) n / knots)) for k = 0 .. knots - 1, in integers."""
    k = np.arange(knots, dtype=np.int64)
    return np.minimum(n - 1, ((2 * k + 1) * n) // (2 * knots))


def quantile_table(s, knots):
    """s: (C, H, W) -> (C, knots), same dtype."""
    C = s.shape[0]
    flat = torch.sort(s.reshape(C, -1), dim=1).values
    return flat[:, torch.from_numpy(quantile_index(flat.shape[1], knots))]


def decide(f, bins, pinned=None):
    """The decisions of one frame f (C, H, W): lo, hi (C,) float32, b (C, N) int64, frac (C, N) float32 - numpy float32 arithmetic, one
    rounding per operation.  `pinned` (C, N): bins decided elsewhere - by another run of the same network whose activations differ in their
    last bits - are taken as given, and frac = clamp(t - b, 0, 1) follows them: an element the other run put on the far side of a bin's edge
    sits at that edge here, so the matched value is the other run's up to rounding (see HistNet.feval)."""
    C = f.shape[0]
    v = f.detach().reshape(C, -1).to(torch.float32).numpy()
    lo, hi = v.min(1), v.max(1)
    span = hi.astype(np.float64) - lo.astype(np.float64)
    inv = np.zeros(C, np.float32)
    inv[hi != lo] = (np.float64(bins) / span[hi != lo]).astype(np.float32)
    t = (v - lo[:, None]).astype(np.float32) * inv[:, None]
    assert t.dtype == np.float32
    if pinned is not None:
        b = np.asarray(pinned, dtype=np.int64).reshape(C, -1)
        assert b.shape == t.shape and b.min() >= 0 and b.max() <= bins - 1
        return lo, hi, b, np.clip(t - b.astype(np.float32), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    b = np.minimum(bins - 1, t.astype(np.int64))
    frac = np.minimum(np.float32(1.0), (t - b.astype(np.float32)).astype(np.float32))
    return lo, hi, b, frac


def state(f, bins, pinned=None):
    """-> (lo (C,) float32, hi (C,) float32, cum (C, bins + 1) int64) as numpy arrays: what maua_feat_hist_fwd leaves in its state."""
    lo, hi, b, _ = decide(f, bins, pinned)
    cnt = np.stack([np.bincount(row, minlength=bins) for row in b])
    cum = np.concatenate([np.zeros((len(cnt), 1), np.int64), np.cumsum(cnt, 1)], 1)
    return lo, hi, cum


def matched(f, table, bins, pinned=None):
    """R (C, H, W) in fp64: f histogram-matched to table (C, K), channel by channel."""
    C, N = f.shape[0], f.shape[1] * f.shape[2]
    K = table.shape[1]
    _, _, b, frac = decide(f, bins, pinned)
    _, _, cum = state(f, bins, pinned)
    rows = np.arange(C)[:, None]
    c0, c1 = cum[rows, b], cum[rows, b + 1]
    q = (c0 + frac.astype(np.float64) * (c1 - c0)) / N
    p = np.clip(q * K - 0.5, 0.0, K - 1.0)
    i0 = np.minimum(K - 2, np.floor(p).astype(np.int64))
    T = table.detach().double().numpy()
    r = T[rows, i0] + (p - i0) * (T[rows, i0 + 1] - T[rows, i0])
    return torch.from_numpy(r).reshape(f.shape)


def term(f, table, bins, pinned=None):
    """h, differentiable in f (R detached); f in fp64 for an fp64 value."""
    return ((f - matched(f, table, bins, pinned).to(f.dtype)) ** 2).mean()


def backward(f, table, bins, coef=None, upstream=1.0):
    """The analytic gradient the kernel implements: coef upstream (F - R), coef = 2 / (C N) where None."""
    coef = 2.0 / f.nelement() if coef is None else coef
    return coef * upstream * (f.detach().double() - matched(f, table, bins))


class HistNet(fr.FlipNet):
    """One image through the loss network whose style modules carry the shift, mirror and feature-histogram terms (cfg.hist_loss_factor,
    cfg.hist_loss_bins, cfg.hist_loss_knots)."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        super().__init__(cfg, state_dict, dtype)
        self.hist_loss_factor = float(getattr(cfg, "hist_loss_factor", 0.0))
        self.bins = int(getattr(cfg, "hist_loss_bins", BINS))
        self.knots = int(getattr(cfg, "hist_loss_knots", KNOTS))
        self.hist_targets = {}

    def capture_style(self, images, blend_weights, style_guides=None):
        super().capture_style(images, blend_weights, None)
        if self.hist_loss_factor <= 0:
            return
        for img, bw in zip(images, blend_weights):
            acts, _ = self.net._forward(img.to(self.dtype))
            for i, l in enumerate(self.spec):
                if l.kind != "style":
                    continue
                t = bw * quantile_table(acts[i][0], self.knots)
                self.hist_targets[i] = t if i not in self.hist_targets else self.hist_targets[i] + t

    def hist_terms(self, x):
        """{spec index: h} of the style layers for the image x (no gradient)."""
        acts, _ = self.net._forward(x.detach().to(self.dtype))
        return {i: float(term(acts[i][0], self.hist_targets[i], self.bins)) for i, l in enumerate(self.spec) if l.kind == "style"}

    def feval(self, x, content_guide=None, pinned=None):
        """-> (total, {spec index: loss}, gradient), by autograd.  `pinned`: {spec index of a style layer: bins (C, N)} decided by the
        run this evaluation is compared with (decide).  The bin of an element is a decision and the matched value is not continuous across
        it: an element that moves from bin b to b + 1 lowers cum[b + 1] by one, so q jumps by up to 1 / N for it and for every element of
        the two bins.  Two runs of one network whose activations differ in the last bits - fp32 kernels and this fp64 restatement - decide a
        few elements per layer differently, and their gradients then differ by 1e-4 .. 1e-3 (the restatement in fp32 against itself in fp64:
        3.6e-4 at 64 x 64 with 256 bins) whatever the arithmetic after the decision.  With the bins pinned the comparison measures that
        arithmetic, as the oracle pinned to the engine's ReLU and pooling decisions does for the network around it."""
        x = x.detach().to(self.dtype).clone().requires_grad_(True)
        acts, _ = self.net._forward(x)
        losses = {}
        for i, l in enumerate(self.spec):
            s = self.strength.get(i, 0.0)
            acc = (lambda t, s=s: _ScaleGradients.apply(t, s)) if l.normalize else (lambda t: t)
            if l.kind == "tv":
                losses[i] = s * ((x[:, :, 1:, :] - x[:, :, :-1, :]).abs().sum() + (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().sum())
            elif l.kind == "content":
                t = self.content_targets[i]
                if acts[i].shape[1:] != t.shape[1:]:
                    continue
                losses[i] = acc(((acts[i] - t) ** 2).mean()) * s
            elif l.kind == "style":
                G, _, _ = self._layer_grams(acts[i], None, l)
                t = ((G[0] - self.style_targets[i][0]) ** 2).mean()
                ts = t
                if self.shift_factor > 0:
                    here = sr.layer_deltas(*acts[i].shape[2:])
                    use = [d for d in self.shift_deltas[i] if d in here]
                    for key, g in self._shift_grams(acts[i], use, l).items():
                        ts = ts + self.shift_factor * ((g - self.shift_targets[i][key]) ** 2).mean()
                for kind in self.kinds:
                    factor = self.rotation_factor if kind == fr.ROT180 else self.flip_factor
                    g = fr.mirrored_gram(acts[i][0], kind, l.use_covariance)
                    ts = ts + factor * ((g - self.flip_targets[i][kind]) ** 2).mean()
                if self.hist_loss_factor > 0:
                    ts = ts + self.hist_loss_factor * term(acts[i][0], self.hist_targets[i], self.bins, (pinned or {}).get(i))
                total = acc(ts) * s
                if l.video_style_factor > 0:
                    total = total + l.video_style_factor * acc(t) * s
                losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build(content, styles, cfg, state_dict, dtype=torch.float64):
    net = HistNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights)
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net


def optimize(content, styles, init, num_iters, cfg, state_dict, dtype=torch.float64):
    """optim.optimize for one image with cfg.hist_loss_factor: the oracle's L-BFGS / Adam drivers over this evaluation."""
    net = build(content, styles, cfg, state_dict, dtype)
    shape = init.shape

    def fg(xf):
        total, _, g = net.feval(xf.reshape(shape))
        return float(total), g.flatten()

    x0 = init.to(dtype)
    if cfg.optimizer == "lbfgs":
        out, _ = lbfgs_run(fg, x0, num_iters, history=cfg.lbfgs_num_correction, tol_grad=float(cfg.lbfgs_tolerance_grad),
                           tol_change=float(cfg.lbfgs_tolerance_change))
    else:
        out, _ = adam_run(fg, x0, num_iters, lr=cfg.learning_rate)
    return out
