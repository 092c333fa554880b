"""The MRF patch-matching style loss (Li & Wand 2016; include/maua_hip.h) restated in fp64 torch.

One frame F (C, H, W), H, W >= 3.  Queries q = yq Wq + xq on the grid Hq = H - 2, Wq = W - 2; the patch of a query is the 3 x 3 window whose
top-left corner it names, flattened in (c, dy, dx) order - which is the row order of `torch.nn.functional.unfold`.  A bank is a style map
S (C, Hs, Ws), origins (P,) = ys Ws + xs and inv (P,) = 1 / ||patch||.

    score(q, p) = inv[p] <patch_q(F), patch_p(S)>;   nn[q] = arg max_p, the lowest p among equal scores
    loss = mean over (q, c, dy, dx) of (patch_q(F) - patch_nn[q](S))^2;   the gradient by autograd with nn held fixed

`gather_gradient` states the same gradient the way the kernel forms it (a gather per element); tests/test_mrf_cpu.py holds the two equal.
The bank builder (`grid`, `build_bank`) restates loss.mrf_grid / StyleLoss's capture: the stride rule, the cap, several maps stacked along
the height and zero-padded to the widest, no patch across two maps, no patch of norm 0.
"""
import torch
import torch.nn.functional as F


def patches(x):
    """(C, H, W) -> (Q, 9 C): row q = yq Wq + xq, columns in (c, dy, dx) order."""
    return F.unfold(x.unsqueeze(0), kernel_size=3)[0].t().contiguous()


def bank_patches(s, origin):
    """The listed patches of the style map s (C, Hs, Ws): (P, 9 C)."""
    ws = s.shape[2]
    o = origin.long()
    ys, xs = o // ws, o % ws
    return patches(s)[ys * (ws - 2) + xs]


def inverse_norms(s, origin):
    """inv (P,) float32: the squared norm in fp64, 1 / sqrt rounded once."""
    return (1.0 / bank_patches(s.double(), origin).pow(2).sum(1).sqrt()).float()


def scores(f, s, origin, inv):
    """(Q, P) fp64."""
    return (patches(f.double()) @ bank_patches(s.double(), origin).t()) * inv.double()[None, :]


def nearest(sc):
    """arg max along p with the lowest index among equal scores."""
    best = sc.max(dim=1, keepdim=True).values
    p = torch.arange(sc.shape[1])[None, :].expand_as(sc)
    return torch.where(sc == best, p, torch.full_like(p, sc.shape[1])).min(dim=1).values


def margins(sc):
    """Per query (best, relative margin between the best and the second-best score; inf with one patch)."""
    top = sc.topk(min(2, sc.shape[1]), dim=1).values
    if sc.shape[1] == 1:
        return top[:, 0], torch.full_like(top[:, 0], float("inf"))
    return top[:, 0], (top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp_min(1e-300)


def loss(f, s, origin, nn):
    d = patches(f.double()) - bank_patches(s.double(), origin)[nn.long()]
    return d.pow(2).mean()


def gradient(f, s, origin, nn, coef=None):
    """coef x d/dF of sum (patch_q(F) - patch_nn[q](S))^2 / 2 ... stated through autograd: the gradient of `loss` is this with
    coef = 2 / (9 C Q), the value loss.py passes."""
    x = f.double().clone().requires_grad_(True)
    d = patches(x) - bank_patches(s.double(), origin)[nn.long()]
    (0.5 * d.pow(2).sum()).backward()
    c, h, w = f.shape
    if coef is None:
        coef = 2.0 / (9 * c * (h - 2) * (w - 2))
    return coef * x.grad


def gather_gradient(f, s, origin, nn, coef=None):
    """The same, element by element: gx[c][y][x] = coef sum over (dy, dx) with (y - dy, x - dx) a query of
    (F[c][y][x] - S[c][origin[nn[(y-dy) Wq + (x-dx)]] + dy Ws + dx])."""
    c, h, w = f.shape
    hq, wq = h - 2, w - 2
    ws = s.shape[2]
    if coef is None:
        coef = 2.0 / (9 * c * hq * wq)
    f64, flat = f.double(), s.double().reshape(c, -1)
    o = origin.long()[nn.long()].reshape(hq, wq)
    g = torch.zeros_like(f64)
    for dy in range(3):
        for dx in range(3):
            at = (o + dy * ws + dx).reshape(-1)
            g[:, dy:dy + hq, dx:dx + wq] += f64[:, dy:dy + hq, dx:dx + wq] - flat[:, at].reshape(c, hq, wq)
    return coef * g


def grid(sizes, stride, max_patches):
    """sizes: [(Hs_i, Ws_i)] of the maps in stacking order.  Returns (s, origins): s the smallest integer >= stride at which the grids of
    all maps together hold at most max_patches patches, origins the list ys Ws + xs in the stacked map (Ws = the widest), map by map, row
    by row."""
    ws = max(w for _, w in sizes)
    s = max(1, int(stride))
    while sum(len(range(0, h - 2, s)) * len(range(0, w - 2, s)) for h, w in sizes) > max_patches:
        s += 1
    origins, top = [], 0
    for h, w in sizes:
        origins += [(top + y) * ws + x for y in range(0, h - 2, s) for x in range(0, w - 2, s)]
        top += h
    return s, origins


def build_bank(maps, stride, max_patches):
    """maps: [(C, Hs_i, Ws_i)].  Returns (S (C, sum Hs_i, max Ws_i) zero-padded on the right, origin (P,) int32 without the patches of norm
    0, inv (P,) float32, the stride used)."""
    c = maps[0].shape[0]
    ws = max(m.shape[2] for m in maps)
    s_map = torch.zeros(c, sum(m.shape[1] for m in maps), ws, dtype=maps[0].dtype)
    top = 0
    for m in maps:
        s_map[:, top:top + m.shape[1], :m.shape[2]] = m
        top += m.shape[1]
    s, origins = grid([(m.shape[1], m.shape[2]) for m in maps], stride, max_patches)
    origin = torch.tensor(origins, dtype=torch.int32)
    keep = bank_patches(s_map.double(), origin).pow(2).sum(1) > 0
    origin = origin[keep]
    return s_map, origin, inverse_norms(s_map, origin), s


# ------------------------------------------------------------------------------------------------------------------------------------
# the whole network: tests/feat_hist_restatement.HistNet (shift, mirror and feature-histogram terms) with the MRF term on the style
# layers named in cfg.mrf_layers
# ------------------------------------------------------------------------------------------------------------------------------------
import feat_hist_restatement as hr  # noqa: E402


class MrfNet(hr.HistNet):
    """cfg.mrf_factor, cfg.mrf_stride (2), cfg.mrf_max_patches (16384), cfg.mrf_layers ("relu3_1,relu4_1").  Blend weights do not enter the
    term, except that a style image of weight 0 gives no patches."""

    def __init__(self, cfg, state_dict, dtype=torch.float64):
        super().__init__(cfg, state_dict, dtype)
        self.mrf_factor = float(getattr(cfg, "mrf_factor", 0.0))
        self.mrf_stride = int(getattr(cfg, "mrf_stride", 2))
        self.mrf_max_patches = int(getattr(cfg, "mrf_max_patches", 16384))
        names = str(getattr(cfg, "mrf_layers", "relu3_1,relu4_1")).split(",")
        self.mrf_slots = []
        for i, l in enumerate(self.spec):
            if l.kind == "style" and self.mrf_factor > 0:
                at = max(k for k in range(i) if self.spec[k].kind in ("relu", "conv"))
                if self.spec[at].name in names:
                    self.mrf_slots.append(i)
        self.mrf_banks = {}

    def capture_style(self, images, blend_weights, style_guides=None):
        super().capture_style(images, blend_weights, None)
        maps = {i: [] for i in self.mrf_slots}
        for img, bw in zip(images, blend_weights):
            if bw == 0:
                continue
            acts, _ = self.net._forward(img.to(self.dtype))
            for i in self.mrf_slots:
                maps[i].extend(acts[i][b].float() for b in range(acts[i].shape[0]))  # the bank holds fp32 values, as the device's does
        for i in self.mrf_slots:
            self.mrf_banks[i] = build_bank(maps[i], self.mrf_stride, self.mrf_max_patches)[:3]

    def mrf_nearest(self, x):
        """{spec index: nn (Q,)} decided by this network in fp64 for the image x."""
        acts, _ = self.net._forward(x.detach().to(self.dtype))
        return {i: nearest(scores(acts[i][0], *self.mrf_banks[i])) for i in self.mrf_slots}

    def mrf_terms(self, x):
        """{spec index: m} with the network's own decisions (no gradient)."""
        acts, _ = self.net._forward(x.detach().to(self.dtype))
        return {i: float(loss(acts[i][0], self.mrf_banks[i][0], self.mrf_banks[i][1], nearest(scores(acts[i][0], *self.mrf_banks[i]))))
                for i in self.mrf_slots}

    def feval(self, x, content_guide=None, pinned=None, nn=None):
        """-> (total, {spec index: loss}, gradient), by autograd: HistNet.feval with mrf_factor m added to a style layer's scalar before
        strength and normalisation apply.  `nn`: {spec index: (frames, Q) decisions} of the run this evaluation is compared with (the
        arg-max is a decision, and the gradient is not continuous across it); None: this network's own.  x may hold several frames: the
        style terms are then per frame, divided by the number of frames (no dynamic term: video_style_factor must be 0)."""
        x = x.detach().to(self.dtype).clone().requires_grad_(True)
        acts, _ = self.net._forward(x)
        frames = x.shape[0]
        losses = {}
        for i, l in enumerate(self.spec):
            s = self.strength.get(i, 0.0)
            acc = (lambda t, s=s: hr._ScaleGradients.apply(t, s)) if l.normalize else (lambda t: t)
            if l.kind == "tv":
                losses[i] = s * ((x[:, :, 1:, :] - x[:, :, :-1, :]).abs().sum() + (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().sum())
            elif l.kind == "content":
                t = self.content_targets[i]
                if acts[i].shape[1:] != t.shape[1:]:
                    continue
                losses[i] = acc(((acts[i] - t) ** 2).mean()) * s
            elif l.kind == "style":
                assert frames == 1 or l.video_style_factor == 0
                total = 0
                for b in range(frames):
                    a = acts[i][b:b + 1]
                    G, _, _ = self._layer_grams(a, None, l)
                    t = ((G[0] - self.style_targets[i][0]) ** 2).mean()
                    ts = t
                    if self.shift_factor > 0:
                        here = hr.sr.layer_deltas(*a.shape[2:])
                        use = [d for d in self.shift_deltas[i] if d in here]
                        for key, g in self._shift_grams(a, use, l).items():
                            ts = ts + self.shift_factor * ((g - self.shift_targets[i][key]) ** 2).mean()
                    for kind in self.kinds:
                        factor = self.rotation_factor if kind == hr.fr.ROT180 else self.flip_factor
                        g = hr.fr.mirrored_gram(a[0], kind, l.use_covariance)
                        ts = ts + factor * ((g - self.flip_targets[i][kind]) ** 2).mean()
                    if self.hist_loss_factor > 0:
                        ts = ts + self.hist_loss_factor * hr.term(a[0], self.hist_targets[i], self.bins, (pinned or {}).get(i))
                    if i in self.mrf_slots:
                        s_map, origin, inv = self.mrf_banks[i]
                        fixed = nn[i][b] if nn is not None else nearest(scores(a[0].detach(), s_map, origin, inv))
                        d = patches(a[0]) - bank_patches(s_map.to(self.dtype), origin)[fixed.long()]
                        ts = ts + self.mrf_factor * d.pow(2).mean()
                    total = total + acc(ts) * s / frames
                    if l.video_style_factor > 0:
                        total = total + l.video_style_factor * acc(t) * s
                losses[i] = total
        total = sum(losses.values())
        total.backward()
        return total.detach(), {i: v.detach() for i, v in losses.items()}, x.grad.detach()


def build_net(content, styles, cfg, state_dict, dtype=torch.float64):
    net = MrfNet(cfg, state_dict, dtype)
    net.capture_content(content)
    net.capture_style(styles, cfg.style_blend_weights)
    if getattr(cfg, "normalize_weights", False):
        net.normalize_weights()
    return net
