"""Restatement of the mirrored-Gram (symmetry) style loss in plain torch, any dtype (the tests use fp64).

Definitions (Berger & Memisevic 2016, the symmetry terms), for one frame of a style layer with activation F (C, H, W):
  mirrors        kind 0 = LR: (y, x) -> (y, W - 1 - x); 1 = UD: (y, x) -> (H - 1 - y, x); 2 = point mirror (rotation by 180 degrees):
                 (y, x) -> (H - 1 - y, W - 1 - x), flat p -> H W - 1 - p;
  mirrored Gram  X = F - mu (mu: the whole map's row means with covariance, else 0),
                 G_m = mirror_m(X) X^T / (C H W) over all pixels - written with torch.flip here; mirrored_gram_flat states the index form
                 sum_p X[c][sigma_m(p)] X[k][p] the kernels use.  Symmetric, since sigma_m is a bijection and its own inverse;
  kinds in use   LR and UD with flip_factor > 0, the point mirror with rotation_factor > 0;
  targets        T_m = sum_i b_i G_m(style_i); every style layer has them, whatever its size;
  loss           t' = t + shift_factor sum_s mse(G_s, T_s) + flip_factor (mse(G_LR, T_LR) + mse(G_UD, T_UD)) + rotation_factor mse(G_180, T_180),
                 t the static scalar; the static term is acc(t') s and the dynamic one (video_style_factor > 0) stays vsf acc(t) s;
  gradient       dL/dX[c][q] = sum_m coef_m sum_k (D_m[c][k] + D_m[k][c]) X[k][sigma_m(q)], D_m = dL/dG_m as given; dL/dF = dL/dX, the term
                 through mu vanishes (sum_q X[k][sigma(q)] = sum_p X[k][p] = 0).
The network around the style layers is oracle.style_oracle's (by way of tests/shift_restatement.py), differentiated by autograd.
"""
import torch

import shift_restatement as sr
from guided_restatement import _ScaleGradients
from oracle.style_oracle import adam_run, lbfgs_run, loss_order  # noqa: F401

LR, UD, ROT180 = 0, 1, 2
FLIP_DIMS = {LR: (2,), UD: (1,), ROT180: (1, 2)}


def centred(f, use_covariance):
    """f: (C, H, W)"""
    return f - f.mean((1, 2), keepdim=True) if use_covariance else f


def mirrored_gram(f, kind, use_covariance=False, normalise=True):
    """f: (C, H, W).  torch.flip."""
    C, H, W = f.shape
    x = centred(f, use_covariance)
    g = torch.flip(x, FLIP_DIMS[kind]).reshape(C, -1) @ x.reshape(C, -1).t()
    return g / (C * H * W) if normalise else g


def sigma(kind, H, W):
    """The mirror as a permutation of the flat pixel index."""
    p = torch.arange(H * W)
    y, x = p // W, p % W
    if kind == LR:
        return y * W + (W - 1 - x)
    if kind == UD:
        return (H - 1 - y) * W + x
    return H * W - 1 - p


def mirrored_gram_flat(f, kind, use_covariance=False):
    """The same matrix from the flat pixel index: sum_p X[c][sigma(p)] X[k][p] / (C H W)."""
    C, H, W = f.shape
    x = centred(f, use_covariance).reshape(C, H * W)
    return x[:, sigma(kind, H, W)] @ x.t() / (C * H * W)


def flip_backward(f, kinds, dmats, use_covariance=False, coefs=None):
    """The analytic gradient the kernels implement: dmats[m] = dL/dG_m (not symmetric) -> dL/dF (C, H, W).  No mean correction."""
    C, H, W = f.shape
    x = centred(f, use_covariance).reshape(C, H * W)
    gx = torch.zeros_like(x)
    for m, (kind, D) in enumerate(zip(kinds, dmats)):
        coef = 1.0 / (C * H * W) if coefs is None else coefs[m]
        gx += coef * ((D + D.t()) @ x[:, sigma(kind, H, W)])
    return gx.reshape(C, H, W)


def kinds_of(flip_factor, rotation_factor):
    return ([LR, UD] if flip_factor > 0 else []) + ([ROT180] if rotation_factor > 0 else [])


class FlipNet(sr.ShiftNet):
    """One image through the loss network whose style modules carry the shift terms (cfg.shift_factor) and the mirror terms
    (cfg.flip_factor, cfg.rotation_factor)."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        super().__init__(cfg, state_dict, dtype)
        self.flip_factor = float(getattr(cfg, "flip_factor", 0.0))
        self.rotation_factor = float(getattr(cfg, "rotation_factor", 0.0))
        self.kinds = kinds_of(self.flip_factor, self.rotation_factor)
        self.flip_targets = {}

    def capture_style(self, images, blend_weights, style_guides=None):
        super().capture_style(images, blend_weights, None)
        if not self.kinds:
            return
        for img, bw in zip(images, blend_weights):
            acts, _ = self.net._forward(img.to(self.dtype))
            for i, l in enumerate(self.spec):
                if l.kind != "style":
                    continue
                prev = self.flip_targets.setdefault(i, {})
                for kind in self.kinds:
                    g = mirrored_gram(acts[i][0], kind, l.use_covariance)
                    prev[kind] = bw * g if kind not in prev else prev[kind] + bw * g

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
                    here = sr.layer_deltas(*acts[i].shape[2:])
                    use = [d for d in self.shift_deltas[i] if d in here]
                    for key, g in self._shift_grams(acts[i], use, l).items():
                        ts = ts + self.shift_factor * ((g - self.shift_targets[i][key]) ** 2).mean()
                for kind in self.kinds:
                    factor = self.rotation_factor if kind == ROT180 else self.flip_factor
                    g = mirrored_gram(acts[i][0], kind, l.use_covariance)
                    ts = ts + factor * ((g - self.flip_targets[i][kind]) ** 2).mean()
                total = acc(ts) * s
                if l.video_style_factor > 0:
                    total = total + l.video_style_factor * acc(t) * s
                losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build(content, styles, cfg, state_dict, dtype=torch.float64):
    net = FlipNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights)
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net


def optimize(content, styles, init, num_iters, cfg, state_dict, dtype=torch.float64):
    """optim.optimize for one image with cfg.flip_factor / cfg.rotation_factor: the oracle's L-BFGS / Adam drivers over this evaluation."""
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
