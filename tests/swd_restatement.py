"""Restatement of the sliced Wasserstein style loss (Heitz, Vanhoey, Chambon & Belcour 2021) on the CPU, as DESIGN.md section 17 writes it:
the projection in fp64, the match, the term, the backward, `decide` and the pinning from tests/feat_hist_restatement.py applied to P.

For one frame F (C, H, W) of a style layer (N = H W), directions V (D, C) with rows of unit length, a target table T (D, K), NB bins:
  directions V of the style layer `index` (its position among the style layers): a CPU torch.Generator seeded with seed * 8191 + index draws
             randn(D, C) in fp64; every row is divided by the square root of its sum of squares in fp64 and rounded to float32 once;
  project    P = V F, (D, H, W), in fp64;
  match      section 15 on P with D in the place of C (feat_hist_restatement.decide / state / matched): range, bin, counts, R;
  term       s = mean over d, i of (P - R)^2, R a constant in the derivative: ds/dF = 2 / (D N) V^T (P - R);
  table      of a style activation S: the quantile table of V S (feat_hist_restatement.quantile_table); several style images add
             blend weight x T;
  loss       t' = t + [shift terms] + [mirror terms] + hist_loss_factor h + swd_factor s; the dynamic term stays vsf acc(t) s.
The network around the style layers is HistNet's.
"""
import numpy as np  # noqa: F401
import torch

import feat_hist_restatement as hr
import flip_restatement as fr
import shift_restatement as sr
from guided_restatement import _ScaleGradients

BINS, KNOTS = 256, 1024  # the defaults of the preset keys swd_bins / swd_knots


def directions(c, d, seed, index):
    """(d, c) float32."""
    gen = torch.Generator()
    gen.manual_seed(seed * 8191 + index)
    v = torch.randn(d, c, dtype=torch.float64, generator=gen)
    length = (v * v).sum(dim=1).sqrt()
    return (v / length[:, None]).float()


def project(f, v):
    """P (D, H, W) = V F in fp64 (differentiable in f)."""
    C, H, W = f.shape
    return (v.double() @ f.double().reshape(C, H * W)).reshape(v.shape[0], H, W)


def table(s, v, knots):
    """The target of one style activation s (C, Hs, Ws)."""
    return hr.quantile_table(project(s, v), knots)


def term(f, v, tab, bins, pinned=None):
    """s, differentiable in f; `pinned` (D, N): bins of P decided elsewhere."""
    return hr.term(project(f, v), tab, bins, pinned)


def residual(p, tab, bins):
    """G = P - R (D, H, W) in fp64 for projections p given as they are (the decisions are taken on p rounded to float32)."""
    return p.detach().double() - hr.matched(p, tab, bins)


def backward(p, v, tab, bins, coef=None, upstream=1.0):
    """coef upstream V^T (P - R) (C, H, W) for projections p, coef = 2 / (D N) where None."""
    D, H, W = p.shape
    coef = 2.0 / p.nelement() if coef is None else coef
    return (coef * upstream * (v.double().t() @ residual(p, tab, bins).reshape(D, H * W))).reshape(v.shape[1], H, W)


class SwdNet(hr.HistNet):
    """One image through the loss network whose style modules carry the shift, mirror, feature-histogram and sliced Wasserstein terms
    (cfg.swd_factor, cfg.swd_directions - 0: as many as channels -, cfg.swd_seed, cfg.swd_bins, cfg.swd_knots)."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        super().__init__(cfg, state_dict, dtype)
        self.swd_factor = float(getattr(cfg, "swd_factor", 0.0))
        self.swd_directions = int(getattr(cfg, "swd_directions", 0))
        self.swd_seed = int(getattr(cfg, "swd_seed", 0))
        self.swd_bins = int(getattr(cfg, "swd_bins", BINS))
        self.swd_knots = int(getattr(cfg, "swd_knots", KNOTS))
        self.swd_targets, self.swd_dirs = {}, {}

    def style_slots(self):
        return [i for i, l in enumerate(self.spec) if l.kind == "style"]

    def capture_style(self, images, blend_weights, style_guides=None):
        super().capture_style(images, blend_weights, None)
        if self.swd_factor <= 0:
            return
        for img, bw in zip(images, blend_weights):
            acts, _ = self.net._forward(img.to(self.dtype))
            for index, i in enumerate(self.style_slots()):
                C = acts[i].shape[1]
                if i not in self.swd_dirs:
                    self.swd_dirs[i] = directions(C, self.swd_directions or C, self.swd_seed, index)
                t = bw * table(acts[i][0], self.swd_dirs[i], self.swd_knots)
                self.swd_targets[i] = t if i not in self.swd_targets else self.swd_targets[i] + t

    def feval(self, x, content_guide=None, pinned=None, swd_pinned=None):
        """HistNet.feval with swd_factor s added to every style layer's static scalar.  `swd_pinned`: {spec index: bins (D, N)} of the
        projections, decided by the run this evaluation is compared with."""
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
                    ts = ts + self.hist_loss_factor * hr.term(acts[i][0], self.hist_targets[i], self.bins, (pinned or {}).get(i))
                if self.swd_factor > 0:
                    ts = ts + self.swd_factor * term(acts[i][0], self.swd_dirs[i], self.swd_targets[i], self.swd_bins, (swd_pinned or {}).get(i))
                total = acc(ts) * s
                if l.video_style_factor > 0:
                    total = total + l.video_style_factor * acc(t) * s
                losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build(content, styles, cfg, state_dict, dtype=torch.float64):
    net = SwdNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights)
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net
