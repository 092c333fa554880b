"""Restatement of the guided (per-region) style loss in plain torch, any dtype (the tests use fp64).

Definitions, for a style layer with activation F (C, N = H_l W_l) and R guides at image resolution with values in [0, 1]:
  layer guides   g_r = the guide resized to (H_l, W_l), bilinear, align_corners=False, size form (source step = fp32(in) / fp32(out), the
                 convention of the project's resize kernel and of ATen);
  region mass    N_r = sum_p g_r[p]^2; a region with N_r < 1 is inactive at that layer;
  guided Gram    G_r = X_r X_r^T / (C N_r), X_r[:, p] = g_r[p] (F[:, p] - mu_r), mu_r = sum_p g_r[p]^2 F[:, p] / N_r with covariance, else 0;
  targets        T_r = sum_i b_i G_r(style_i) / sum_{i: r active in style i} b_i; no target for a region active in no style image;
  loss           per active region with a target, t_r = mean((G_r - T_r)^2):  acc(t_r) s + [vsf > 0] vsf acc(t_r) s, acc = ScaleGradients when
                 `normalize`;  --normalize_weights divides s by C.
  gradient       dL/dF[:, p] = sum_r (2 / (C N_r)) g_r[p]^2 D_r (F[:, p] - mu_r), D_r = dL/dG_r symmetric.
The network around the style layers (convolutions, ReLUs, pools, content / TV terms) is oracle.style_oracle's, differentiated by autograd.
"""
import numpy as np
import torch

from oracle.style_oracle import OracleNet, adam_run, build_spec, lbfgs_run, loss_order  # noqa: F401


def resize_guides(guide, hl, wl, dtype=torch.float64):
    """(R, H, W) -> (R, hl, wl): bilinear, align_corners=False, source step fp32(H) / fp32(hl)."""
    guide = guide.to(dtype)
    R, H, W = guide.shape

    def axis(out, size):
        scale = float(np.float32(size) / np.float32(out))
        s = torch.clamp(scale * (torch.arange(out, dtype=torch.float64) + 0.5) - 0.5, min=0.0)
        i0 = torch.clamp(s.floor().long(), max=size - 1)
        i1 = torch.clamp(i0 + 1, max=size - 1)
        return i0, i1, (s - i0.double()).to(dtype)

    y0, y1, ly = axis(int(hl), H)
    x0, x1, lx = axis(int(wl), W)
    top = guide[:, y0][:, :, x0] * (1 - lx) + guide[:, y0][:, :, x1] * lx
    bot = guide[:, y1][:, :, x0] * (1 - lx) + guide[:, y1][:, :, x1] * lx
    return top * (1 - ly)[None, :, None] + bot * ly[None, :, None]


def region_mass(g):
    """g: (R, N) -> N_r (R,)"""
    return (g * g).sum(1)


def guided_grams(f, g, use_covariance=False):
    """f: (C, N), g: (R, N) -> (G (R, C, C), mass (R,), active [R]).  Inactive regions: zeros."""
    C = f.shape[0]
    mass = region_mass(g)
    active = [bool(m >= 1.0) for m in mass]
    out = []
    for r in range(g.shape[0]):
        if not active[r]:
            out.append(torch.zeros(C, C, dtype=f.dtype))
            continue
        fc = f
        if use_covariance:
            mu = (f * (g[r] * g[r])[None, :]).sum(1) / mass[r]
            fc = f - mu[:, None]
        x = fc * g[r][None, :]
        out.append(x @ x.t() / (C * mass[r]))
    return torch.stack(out), mass, active


def guided_grad(f, g, d, use_covariance=False):
    """The analytic gradient: d (R, C, C) = dL/dG_r, symmetric -> dL/dF (C, N)."""
    C = f.shape[0]
    mass = region_mass(g)
    gf = torch.zeros_like(f)
    for r in range(g.shape[0]):
        if mass[r] < 1.0:
            continue
        w = g[r] * g[r]
        mu = (f * w[None, :]).sum(1) / mass[r] if use_covariance else torch.zeros(C, dtype=f.dtype)
        gf = gf + (2.0 / (C * mass[r])) * (d[r] @ (f - mu[:, None])) * w[None, :]
    return gf


class _ScaleGradients(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, strength):
        ctx.strength = strength
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g / (g.norm() + 1e-8) * ctx.strength * ctx.strength, None


class GuidedNet:
    """One image through the loss network with guided style modules.  guides=None everywhere restates the unguided modules."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        self.cfg, self.dtype = cfg, dtype
        self.spec = build_spec(cfg)
        self.net = OracleNet(self.spec, state_dict, dtype)
        self.strength = {i: l.strength for i, l in enumerate(self.spec) if l.kind in ("content", "style", "tv", "temporal")}
        self.content_targets, self.style_targets, self.style_has = {}, {}, {}
        self.skipped = []  # (layer index, region) without a target

    def _layer_grams(self, act, guide, l):
        C, H, W = act.shape[1:]
        f = act.reshape(C, H * W)
        if guide is None:
            g = torch.ones(1, H * W, dtype=self.dtype)
        else:
            g = resize_guides(guide, H, W, self.dtype).reshape(guide.shape[0], -1)
        return guided_grams(f, g, l.use_covariance)

    def capture_content(self, image):
        acts, _ = self.net._forward(image.to(self.dtype))
        for i, l in enumerate(self.spec):
            if l.kind == "content":
                self.content_targets[i] = acts[i].detach().clone()

    def capture_style(self, images, blend_weights, style_guides=None):
        sums, weights = {}, {}
        for k, (img, bw) in enumerate(zip(images, blend_weights)):
            acts, _ = self.net._forward(img.to(self.dtype))
            for i, l in enumerate(self.spec):
                if l.kind != "style":
                    continue
                G, _, active = self._layer_grams(acts[i], None if style_guides is None else style_guides[k], l)
                w = torch.tensor([bw if a else 0.0 for a in active], dtype=self.dtype)
                sums[i] = bw * G if i not in sums else sums[i] + bw * G
                weights[i] = w if i not in weights else weights[i] + w
        for i in sums:
            self.style_has[i] = [bool(w > 0) for w in weights[i]]
            inv = torch.tensor([1.0 / float(w) if w > 0 else 0.0 for w in weights[i]], dtype=self.dtype)
            self.style_targets[i] = sums[i] * inv[:, None, None]
            self.skipped += [(i, r) for r, h in enumerate(self.style_has[i]) if not h]

    def normalize_weights(self):
        for i, l in enumerate(self.spec):
            if l.kind == "content":
                self.strength[i] = self.strength[i] / max(self.content_targets[i].shape)
            elif l.kind == "style":
                self.strength[i] = self.strength[i] / self.style_targets[i].shape[-1]

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
                G, _, active = self._layer_grams(acts[i], content_guide, l)
                vsf = l.video_style_factor
                total = 0
                for r in range(G.shape[0]):
                    if not (active[r] and self.style_has[i][r]):
                        continue
                    t_r = ((G[r] - self.style_targets[i][r]) ** 2).mean()
                    total = total + acc(t_r) * s
                    if vsf > 0:
                        total = total + vsf * acc(t_r) * s
                if torch.is_tensor(total):
                    losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build(content, styles, cfg, state_dict, guides=None, dtype=torch.float64):
    """The net with its targets captured, as optim.optimize prepares it.  guides = (content guide, [style guides]) or None."""
    net = GuidedNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights, None if guides is None else guides[1])
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net


def optimize(content, styles, init, num_iters, cfg, state_dict, guides=None, dtype=torch.float64):
    """optim.optimize(..., guides=...) for one image: the oracle's L-BFGS / Adam drivers over this evaluation."""
    net = build(content, styles, cfg, state_dict, guides, dtype)
    shape = init.shape
    cg = None if guides is None else guides[0]

    def fg(xf):
        total, _, g = net.feval(xf.reshape(shape), cg)
        return float(total), g.flatten()

    x0 = init.to(dtype)
    if cfg.optimizer == "lbfgs":
        out, _ = lbfgs_run(fg, x0, num_iters, history=cfg.lbfgs_num_correction, tol_grad=float(cfg.lbfgs_tolerance_grad),
                           tol_change=float(cfg.lbfgs_tolerance_change))
    else:
        out, _ = adam_run(fg, x0, num_iters, lr=cfg.learning_rate)
    return out
