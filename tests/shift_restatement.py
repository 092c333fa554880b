"""Restatement of the shifted-Gram (long-range consistency) style loss in plain torch, any dtype (the tests use fp64).

Definitions (Berger & Memisevic 2016), for one frame of a style layer with activation F (C, H, W):
  deltas(n)      4 ** range(1, int(log2(n) / 2 - 0.5)) on the shorter side n = min(H, W);
  shifts         every delta along x, then along y: (4, x), (4, y), (16, x), (16, y), ...;
  shifted Gram   X = F - mu (mu: the whole map's row means with covariance, else 0),
                 G_(d,x) = X[:, :, d:] X[:, :, :W-d]^T / (C H (W - d)),  G_(d,y) = X[:, d:, :] X[:, :H-d, :]^T / (C (H - d) W)  - written with
                 slices here; the kernels use the flat form p + offset (shifted_gram_flat below states that one);
  targets        T_s = sum_i b_i G_s(style_i); a delta is used when every style image and the working layer produce it;
  loss           t' = t + shift_factor sum_s mean((G_s - T_s)^2), t the static scalar of the unguided module; the static term is acc(t') s and the
                 dynamic one (video_style_factor > 0) stays vsf acc(t) s.
The network around the style layers is oracle.style_oracle's (by way of tests/guided_restatement.py), differentiated by autograd.
"""
import numpy as np
import torch

from guided_restatement import GuidedNet, _ScaleGradients
from oracle.style_oracle import adam_run, lbfgs_run, loss_order  # noqa: F401


def deltas(n):
    return [int(d) for d in 4 ** np.array(range(1, int(np.log2(n) / 2 - 0.5)))] if n >= 1 else []


def layer_deltas(h, w):
    return deltas(min(h, w))


def centred(f, use_covariance):
    """f: (C, H, W)"""
    return f - f.mean((1, 2), keepdim=True) if use_covariance else f


def shifted_gram(f, axis, d, use_covariance=False, normalise=True):
    """f: (C, H, W); axis 0 = x, 1 = y.  Slices."""
    C, H, W = f.shape
    x = centred(f, use_covariance)
    if axis == 0:
        a, b, n = x[:, :, d:], x[:, :, :W - d], H * (W - d)
    else:
        a, b, n = x[:, d:, :], x[:, :H - d, :], (H - d) * W
    g = a.reshape(C, -1) @ b.reshape(C, -1).t()
    return g / (C * n) if normalise else g


def shifted_gram_flat(f, axis, d, use_covariance=False):
    """The same matrix from the flat pixel index: sum over the valid p of X[c][p + off] X[k][p] / (C n_s)."""
    C, H, W = f.shape
    x = centred(f, use_covariance).reshape(C, H * W)
    p = torch.arange(H * W)
    if axis == 0:
        off, valid = d, (p % W) < W - d
    else:
        off, valid = d * W, p < (H - d) * W
    pv = p[valid]
    return x[:, pv + off] @ x[:, pv].t() / (C * int(valid.sum()))


def shift_backward(f, shifts, dmats, use_covariance=False):
    """The analytic gradient the kernels implement: dmats[s] = dL/dG_s (not symmetric) -> dL/dF (C, H, W)."""
    C, H, W = f.shape
    x = centred(f, use_covariance).reshape(C, H * W)
    p = torch.arange(H * W)
    gx = torch.zeros_like(x)
    for (axis, d), D in zip(shifts, dmats):
        off, valid = (d, (p % W) < W - d) if axis == 0 else (d * W, p < (H - d) * W)
        pv = p[valid]
        coef = 1.0 / (C * int(valid.sum()))
        gx[:, pv + off] += coef * (D @ x[:, pv])
        gx[:, pv] += coef * (D.t() @ x[:, pv + off])
    if use_covariance:
        gx = gx - gx.mean(1, keepdim=True)
    return gx.reshape(C, H, W)


class ShiftNet(GuidedNet):
    """One image through the loss network whose style modules carry the shift terms (cfg.shift_factor)."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        super().__init__(cfg, state_dict, dtype)
        self.shift_factor = float(getattr(cfg, "shift_factor", 0.0))
        self.shift_targets, self.shift_deltas, self.dropped = {}, {}, {}

    def _shift_grams(self, act, ds, l):
        return {(d, axis): shifted_gram(act[0], axis, d, l.use_covariance) for d in ds for axis in (0, 1)}

    def capture_style(self, images, blend_weights, style_guides=None):
        super().capture_style(images, blend_weights, None)
        if self.shift_factor <= 0:
            return
        offered = {}
        for img, bw in zip(images, blend_weights):
            acts, _ = self.net._forward(img.to(self.dtype))
            for i, l in enumerate(self.spec):
                if l.kind != "style":
                    continue
                ds = layer_deltas(*acts[i].shape[2:])
                offered.setdefault(i, []).append(ds)
                for key, g in self._shift_grams(acts[i], ds, l).items():
                    prev = self.shift_targets.setdefault(i, {})
                    prev[key] = bw * g if key not in prev else prev[key] + bw * g
        for i, lists in offered.items():
            self.shift_deltas[i] = [d for d in lists[0] if all(d in ds for ds in lists)]
            self.dropped[i] = sorted(set(d for ds in lists for d in ds) - set(self.shift_deltas[i]))

    def feval(self, x, content_guide=None):
        """-> (total, {spec index: loss}, gradient), by autograd."""
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
                    here = layer_deltas(*acts[i].shape[2:])
                    use = [d for d in self.shift_deltas[i] if d in here]
                    for key, g in self._shift_grams(acts[i], use, l).items():
                        ts = ts + self.shift_factor * ((g - self.shift_targets[i][key]) ** 2).mean()
                total = acc(ts) * s
                if l.video_style_factor > 0:
                    total = total + l.video_style_factor * acc(t) * s
                losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build(content, styles, cfg, state_dict, dtype=torch.float64):
    net = ShiftNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights)
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net


def optimize(content, styles, init, num_iters, cfg, state_dict, dtype=torch.float64):
    """optim.optimize for one image with cfg.shift_factor: the oracle's L-BFGS / Adam drivers over this evaluation."""
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
