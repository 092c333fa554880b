"""Loss modules with the reference's names and attributes (reference loss.py), computing on MI355X.

Every tensor-sized operation goes through libmaua_hip (hip.py): Gram / covariance matrices on the fp32
matrix cores, fused MSE forward+backward, total variation.  The modules keep the reference's protocol -
they sit inside the feature network, return their input unchanged and leave the scalar in `.loss`
(`mode` in {"none", "capture", "loss"}) - so code written against the reference's loss.py keeps working,
including autograd: each op is a torch.autograd.Function whose backward is again a HIP kernel.

The iteration loop itself does not run these modules one by one: optim.optimize hands the assembled
network to engine.StyleEngine, which reads `.target`, `.strength`, `.normalize` ... from them and
chains the kernels without autograd.  Both paths produce the same numbers (tests/test_engine_gpu.py).

Spatial control (not in the reference): a StyleLoss with `guide` set matches one Gram matrix per region of the guides
(Gatys et al. 2017; csrc/gram_guided.hip).  Such a network runs through these modules only, unless the planner
field guided_engine is on (then engine.StyleEngine evaluates it; targets are still captured here).

Long-range consistency (--shift_factor; Berger & Memisevic 2016): with `shift_factor > 0` a StyleLoss also matches the products of the
activation with translated copies of itself (csrc/gram_shift.hip).  Such a network runs through these modules only.

Symmetry (the same paper's other half): with `flip_factor > 0` a StyleLoss also matches the products of the activation with its left-right
and its up-down mirror image, with `rotation_factor > 0` the product with its point mirror (rotation by 180 degrees; csrc/gram_flip.hip,
DESIGN.md section 13).  Module path only, like the shift terms.

Feature histograms (Risser, Wilmot & Barnes 2017): with `hist_loss_factor > 0` a StyleLoss also histogram-matches every channel of the
activation to the style's channel and adds the mean squared distance to the matched map (csrc/feat_hist.hip) - the
one term here that is not a second-order statistic.  Module path only.

MRF patch matching (Li & Wand 2016): with `mrf_factor > 0` a StyleLoss also pulls every 3x3 patch of the activation towards its nearest
style patch under normalised cross-correlation and adds the mean squared distance (csrc/mrf.hip) - the one term here
that keeps local structure.  Module path only.

Sliced Wasserstein distance (Heitz, Vanhoey, Chambon & Belcour 2021): with `swd_factor > 0` a StyleLoss also projects the activation's feature
vectors onto `swd_directions` fixed unit directions and matches every projection to the style's by monotone rearrangement - the feature-
histogram match behind a rotation (csrc/swd.hip) - the one term here that constrains the joint distribution of the
channels.  Module path only.
"""
import sys

import numpy as np  # noqa: F401  (kept importable like the reference module)
import torch
import torch.nn as nn

import hip
from utils import info  # noqa: F401


class ScaleGradients(torch.autograd.Function):
    """Identity in the forward pass; the backward pass replaces the incoming gradient g by
    g / (||g|| + 1e-8) * strength^2  (reference loss.py:10-20).  It is applied to the *scalar* MSE, so the
    gradient weight of a loss becomes +-strength^2 whatever the reported weight is."""

    @staticmethod
    def forward(ctx, input_tensor, strength):
        ctx.strength = strength
        return input_tensor

    @staticmethod
    def backward(ctx, grad_output):
        unit = grad_output / (torch.norm(grad_output, keepdim=True) + 1e-8)
        return unit * ctx.strength * ctx.strength, None


def normalize_weights(content_losses, style_losses):
    """Divide every strength by the largest dimension of its target (reference loss.py:24-28)."""
    for mod in list(content_losses) + list(style_losses):
        mod.strength = mod.strength / target_dim(mod)


def target_dim(mod):
    """Largest dimension of a module's target; for a guided StyleLoss that of ONE region's target (its channel count)."""
    if getattr(mod, "guide", None) is not None and mod.guided_target is not None:
        return mod.guided_target.shape[-1]
    return max(mod.target.size())


class _MseFn(torch.autograd.Function):
    """mean((x - target)^2) with the gradient 2 (x - target) / n produced by the same kernel pass."""

    @staticmethod
    def forward(ctx, x, target):
        xc = x.contiguous()
        tc = target.expand_as(x).contiguous()
        n = xc.numel()
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        grad = torch.empty_like(xc)
        hip.mse_fwd_bwd(xc, tc, grad, 1.0 / n, 2.0 / n, False, loss)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


class _GramFn(torch.autograd.Function):
    """X X^T of X = x.reshape(B*C, H*W) (rows optionally centred); backward (dG + dG^T) X."""

    @staticmethod
    def forward(ctx, x, use_covariance):
        B, C, H, W = x.shape
        xc = x.contiguous()
        gram, mean = hip.gram_fwd(xc.reshape(1, B * C, H, W), 1.0, bool(use_covariance))
        ctx.save_for_backward(xc)
        ctx.mean = mean
        return gram

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        d = (g + g.t()).contiguous()
        gf = torch.empty_like(xc)
        hip.gram_bwd(d, xc, ctx.mean, gf, False)
        return gf, None


class _GuidedGramFn(torch.autograd.Function):
    """G_r = scale_r X_r X_r^T for the R guides of a layer, X_r = g_r (x - mu_r) (mu_r: the g_r^2-weighted row means in the covariance
    form, else 0); backward sum_r scale_r g_r^2 (dG_r + dG_r^T) (x - mu_r) - the term through mu_r vanishes, the weighted residuals
    sum to zero."""

    @staticmethod
    def forward(ctx, x, guides, scale, mass, use_covariance):
        B, C, H, W = x.shape
        xc = x.contiguous()
        grams, mean = hip.gram_guided_fwd(xc.reshape(1, B * C, H, W), guides, scale, bool(use_covariance), mass)
        ctx.save_for_backward(xc, guides, scale)
        ctx.mean = mean
        return grams

    @staticmethod
    def backward(ctx, g):
        xc, guides, scale = ctx.saved_tensors
        d = (g + g.transpose(1, 2)).contiguous()
        gf = torch.empty_like(xc)
        hip.gram_guided_bwd(d, xc, guides, scale, ctx.mean, gf, False)
        return gf, None, None, None, None


def shift_deltas(h, w):
    """The translations of a style layer of h x w pixels: the reference's list 4 ** range(1, int(log2(n) / 2 - 0.5)) on the shorter side n
    ([] below 32, [4] up to 127, [4, 16] up to 511, ...; every delta <= n / 8)."""
    n = min(int(h), int(w))
    if n < 1:
        return []
    return [int(d) for d in 4 ** np.array(range(1, int(np.log2(n) / 2 - 0.5)))]


def shift_pairs(axis, delta, h, w):
    """Number of pixel pairs (p, p + offset) of the shift inside an h x w map."""
    return h * (w - delta) if axis == 0 else (h - delta) * w


class _ShiftGramFn(torch.autograd.Function):
    """G_s[c][k] = scale_s sum_p X[c][p + off_s] X[k][p] for the shifts [(axis, delta), ...] of one frame x (1, C, H, W), X = x - mu (mu: the
    map's row means in the covariance form, else 0), over the pairs inside the map; scale_s = 1 / (C n_s) where `scales` is None (apply takes all four arguments).
    Backward: hip.gram_shift_bwd (dL/dX) and, in the covariance form, minus its row means - the crops do not sum to zero."""

    @staticmethod
    def forward(ctx, x, shifts, use_covariance, scales):
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("shifted Gram matrices: one frame per call (B = 1)")
        shifts = [(int(a), int(d)) for a, d in shifts]
        if scales is None:
            scales = [1.0 / (C * shift_pairs(a, d, H, W)) for a, d in shifts]
        xc = x.contiguous()
        mean = None
        if use_covariance:
            mean = torch.empty(C, device=x.device, dtype=torch.float32)
            hip.gram_row_means(xc, mean, hip._ws(None, hip.gram_workspace_bytes(C, H * W), x.device))
        grams = hip.gram_shift_fwd(xc, shifts, scales, mean)
        ctx.save_for_backward(xc)
        ctx.mean, ctx.shifts, ctx.scales = mean, shifts, list(scales)
        return grams

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        gx = torch.empty_like(xc)
        hip.gram_shift_bwd(g.contiguous(), xc, ctx.shifts, ctx.scales, ctx.mean, gx, False)
        if ctx.mean is not None:
            C, hw = xc.shape[1], xc.shape[2] * xc.shape[3]
            rm = torch.empty(C, device=xc.device, dtype=torch.float32)
            hip.gram_row_means(gx, rm, hip._ws(None, hip.gram_workspace_bytes(C, hw), xc.device))
            gx = gx - rm.reshape(1, C, 1, 1)
        return gx, None, None, None


MIRROR_LR, MIRROR_UD, MIRROR_180 = 0, 1, 2  # the kinds of csrc/gram_flip.hip


class _FlipGramFn(torch.autograd.Function):
    """G_m[c][k] = scale_m sum_p X[c][sigma_m(p)] X[k][p] for the mirrors `kinds` (0 = LR, 1 = UD, 2 = point mirror) of one frame x
    (1, C, H, W), over all pixels, X = x - mu (mu: the map's row means in the covariance form, else 0); scale_m = 1 / (C H W) where `scales` is
    None (apply takes all four arguments).  Symmetric, bit for bit.  Backward: hip.gram_flip_bwd alone - a mirror permutes the pixels, so the
    centred rows still sum to zero and the term through the means vanishes."""

    @staticmethod
    def forward(ctx, x, kinds, use_covariance, scales):
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("mirrored Gram matrices: one frame per call (B = 1)")
        kinds = [int(k) for k in kinds]
        if scales is None:
            scales = [1.0 / (C * H * W)] * len(kinds)
        xc = x.contiguous()
        mean = None
        if use_covariance:
            mean = torch.empty(C, device=x.device, dtype=torch.float32)
            hip.gram_row_means(xc, mean, hip._ws(None, hip.gram_workspace_bytes(C, H * W), x.device))
        grams = hip.gram_flip_fwd(xc, kinds, scales, mean)
        ctx.save_for_backward(xc)
        ctx.mean, ctx.kinds, ctx.scales = mean, kinds, list(scales)
        return grams

    @staticmethod
    def backward(ctx, g):
        (xc,) = ctx.saved_tensors
        gx = torch.empty_like(xc)
        hip.gram_flip_bwd(g.contiguous(), xc, ctx.kinds, ctx.scales, ctx.mean, gx, False)
        return gx, None, None, None


class _FeatHistFn(torch.autograd.Function):
    """h = mean (x - R)^2 for one frame x (1, C, H, W): R is x histogram-matched, channel by channel, to the quantile table `table`
    (C, knots) over `bins` bins (hip.feat_hist_fwd).  R is a constant in the derivative: backward is 2 (x - R) / (C H W) times the incoming
    gradient, which hip.feat_hist_bwd reads on the device."""

    @staticmethod
    def forward(ctx, x, table, bins):
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("feature histograms: one frame per call (B = 1)")
        xc = x.contiguous()
        loss, state = hip.feat_hist_fwd(xc, table, int(bins))
        ctx.save_for_backward(xc, table, state)
        ctx.bins = int(bins)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        xc, table, state = ctx.saved_tensors
        gx = torch.empty_like(xc)
        hip.feat_hist_bwd(xc, table, state, ctx.bins, 2.0 / xc.numel(), gx, False, upstream=g.reshape(1).float().contiguous())
        return gx, None, None


class _MrfFn(torch.autograd.Function):
    """m = mean over the queries q and (c, dy, dx) of (Psi_q(x) - Psi_nn[q](S))^2 for one frame x (1, C, H, W): nn[q] is the style patch of
    the bank (s, origin, inv) with the largest normalised cross-correlation to the 3x3 patch Psi_q(x) (hip.mrf_fwd).  nn is a constant in
    the derivative: backward is a gather per element, 2 / (9 C Q) times the incoming gradient (hip.mrf_bwd)."""

    @staticmethod
    def forward(ctx, x, s, origin, inv):
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("MRF patch matching: one frame per call (B = 1)")
        xc = x.contiguous()
        loss, state = hip.mrf_fwd(xc, s, origin, inv)
        ctx.save_for_backward(xc, s, origin, state)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        xc, s, origin, state = ctx.saved_tensors
        _, C, H, W = xc.shape
        gx = torch.empty_like(xc)
        hip.mrf_bwd(xc, s, origin, state, 2.0 / (9.0 * C * (H - 2) * (W - 2)), gx, False, upstream=g.reshape(1).float().contiguous())
        return gx, None, None, None


def swd_directions(c, d, seed, index):
    """The d directions of the style layer `index` (its position in net.style_losses) with c channels: (d, c) float32 on the CPU, rows of
    unit length - a function of (seed, index, c, d) alone.  A CPU generator seeded with seed * 8191 + index draws randn(d, c) in fp64; the
    rows are normalised in fp64 and rounded once.  These fp32 values are the directions for every user of them."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed) * 8191 + int(index))
    v = torch.randn(int(d), int(c), dtype=torch.float64, generator=gen)
    return (v / v.norm(dim=1, keepdim=True)).to(torch.float32)


class _SwdFn(torch.autograd.Function):
    """s = mean (P - R)^2 for one frame x (1, C, H, W): P = dirs x its projections onto the rows of `dirs` (D, C), R the projections matched,
    direction by direction, to the quantile table `table` (D, knots) over `bins` bins.  hip.swd_project and hip.swd_match are looked up on
    the module at every call (a test records P between them); the second leaves G = P - R in P's buffer, which is all the backward needs:
    2 / (D H W) dirs^T G times the incoming gradient (hip.swd_bwd; `dirs_t` (C, D) is the transpose)."""

    @staticmethod
    def forward(ctx, x, dirs, dirs_t, table, bins):
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("sliced Wasserstein distance: one frame per call (B = 1)")
        xc = x.contiguous()
        proj, state, workspace = hip.swd_project(xc, dirs, int(bins))
        loss = hip.swd_match(proj, table, state, int(bins), workspace)
        ctx.save_for_backward(proj, dirs_t)
        ctx.shape = tuple(xc.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        resid, dirs_t = ctx.saved_tensors
        gx = torch.empty(ctx.shape, dtype=torch.float32, device=resid.device)
        hip.swd_bwd(resid, dirs_t, 2.0 / resid.numel(), gx, False, upstream=g.reshape(1).float().contiguous())
        return gx, None, None, None, None


def mrf_grid(sizes, stride, max_patches):
    """The patch grid of a bank over style maps of sizes [(Hs_i, Ws_i)], stacked along the height of one map as wide as the widest:
    (s, origins) - s the smallest integer >= stride at which the grids of all maps together hold at most max_patches patches (a map of
    Hs x Ws has ceil((Hs - 2) / s) ceil((Ws - 2) / s)), origins the host list of ys Ws + xs, map by map and row by row.  Every patch lies
    within one map: none reaches into the next map or into a narrower map's padding."""
    if not sizes or any(h < 3 or w < 3 for h, w in sizes):
        raise ValueError(f"MRF patch matching: style activations of at least 3 x 3 are needed, got {sizes}")
    if int(max_patches) < len(sizes):
        raise ValueError(f"MRF patch matching: mrf_max_patches = {max_patches} for {len(sizes)} style maps")
    ws = max(w for _, w in sizes)
    s = max(1, int(stride))
    while sum(-(-(h - 2) // s) * -(-(w - 2) // s) for h, w in sizes) > int(max_patches):
        s += 1
    origins, top = [], 0
    for h, w in sizes:
        for y in range(0, h - 2, s):
            origins.extend((top + y) * ws + x for x in range(0, w - 2, s))
        top += h
    return s, origins


class LayerGuides:
    """The guides of one style layer: `g` (R, H_l W_l) = the image-resolution guides resized to the activation with the project's bilinear
    kernel, `mass` N_r = sum g_r^2 (device, fp64; `mass_host` its one read-back), `active` = [N_r >= 1] and `scale` = 1 / (C N_r) on the
    device, 0 for an inactive region."""

    def __init__(self, guide, channels, hl, wl):
        g = hip.resize_bilinear(guide.unsqueeze(0).float().contiguous(), size=(int(hl), int(wl)))[0]
        self.g = g.reshape(g.shape[0], -1).contiguous()
        self.mass = hip.gram_guided_mass(self.g)
        self.mass_host = [float(v) for v in self.mass.cpu()]
        self.active = [m >= 1.0 for m in self.mass_host]
        self.scale = torch.tensor([1.0 / (channels * m) if a else 0.0 for m, a in zip(self.mass_host, self.active)],
                                  dtype=torch.float64).to(device=guide.device, dtype=torch.float32)


class _TVFn(torch.autograd.Function):
    """sum |x[:,:,1:,:]-x[:,:,:-1,:]| + sum |x[:,:,:,1:]-x[:,:,:,:-1]| and its sign() gradient, one kernel."""

    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        grad = torch.empty_like(xc)
        hip.tv_fwd_bwd(xc, grad, 1.0, False, loss)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g


class ContentLoss(nn.Module):
    """Feature-space MSE against a captured target (reference loss.py:32-64).  Also used on the pixels as the
    'temporal' loss, with optional per-pixel `weights`."""

    def __init__(self, strength, normalize=False):
        super().__init__()
        self.strength = strength
        self.crit = _MseFn.apply
        self.mode = "none"
        self.weights = None
        self.normalize = normalize
        self.loss = 0
        self.target = torch.Tensor()

    def forward(self, input):
        if self.mode == "none" or (input.shape[1:] != self.target.shape[1:] and self.target.nelement() != 0):
            return input
        if "temporal" in self.name and self.target.shape[0] == 0 and self.mode == "loss":
            return input
        self.loss = 0
        frames = input.shape[0]
        for idx in range(frames):
            if self.mode == "loss":
                frame = input[[idx]]
                if self.weights is not None:
                    frame = frame * self.weights
                loss = self.crit(frame, self.target)
                if self.normalize:
                    loss = ScaleGradients.apply(loss, self.strength)
                self.loss += loss * self.strength / frames
            if self.mode == "capture":
                self.target = input.detach()
        return input


class GramMatrix(nn.Module):
    """(B*C) x (B*C) Gram matrix of a feature batch, or its covariance form (reference loss.py:67-91).  With exactly one of
    `shift_x` / `shift_y` nonzero (one frame, B = 1): the raw shifted product X_A X_B^T of the map with itself translated by that many
    pixels along the axis, X_A[c] = X[c] at p + offset, X_B[k] = X[k] at p, over the pairs inside the map (not symmetric; X is centred on
    the whole map's row means in the covariance form).  With `flip_h` (one frame): the raw product of the map's left-right mirror image
    with the map, sum_p X[c][sigma(p)] X[k][p] over all pixels; `flip_v`: the up-down mirror; both: the point mirror (rotation by 180
    degrees).  These are symmetric.  A flip together with a shift raises.  The reference's own code for these arguments always ends with
    y = x (and its `::-1` slices are illegal in torch); `shift_t` is accepted and has no effect."""

    def forward(self, x, shift_x=0, shift_y=0, shift_t=0, flip_h=False, flip_v=False, use_covariance=False):
        if flip_h or flip_v:
            if shift_x or shift_y:
                raise ValueError("GramMatrix: a flip and a shift together are not defined")
            if x.shape[0] != 1:
                raise ValueError("GramMatrix: a mirrored product needs one frame (B = 1)")
            kind = MIRROR_180 if flip_h and flip_v else MIRROR_LR if flip_h else MIRROR_UD
            return _FlipGramFn.apply(x, [kind], use_covariance, [1.0])[0]
        if shift_x or shift_y:
            if shift_x and shift_y:
                raise ValueError("GramMatrix: one of shift_x / shift_y at a time")
            if x.shape[0] != 1:
                raise ValueError("GramMatrix: a shifted product needs one frame (B = 1)")
            shift = (0, int(shift_x)) if shift_x else (1, int(shift_y))
            return _ShiftGramFn.apply(x, [shift], use_covariance, [1.0])[0]
        return _GramFn.apply(x, use_covariance)


class StyleLoss(nn.Module):
    """Gram-matrix MSE against blended style targets (reference loss.py:94-186): a per-frame 'static' term
    and, when video_style_factor > 0 (the default, 100), a whole-batch 'dynamic' term.

    Per frame the static scalar t = mse(G, T) becomes t + shift_factor sum_s mse(G_s, T_s) + flip_factor (mse(G_LR, T_LR) + mse(G_UD, T_UD))
    + rotation_factor mse(G_180, T_180): the shifted products of DESIGN.md section 12 and the mirrored ones of section 13.  `rotation_factor`
    drives the 180 degree term only; the paper's 90 degree terms (square maps, a transposing read) are not implemented.  With
    `hist_loss_factor > 0` the scalar also gains hist_loss_factor h, h the feature-histogram term of DESIGN.md section 15 (`hist_loss_bins`
    bins, a target of `hist_loss_knots` quantiles per channel; use_covariance does not change it).  With `mrf_factor > 0` it gains
    mrf_factor m, m the MRF patch-matching term of DESIGN.md section 16: the bank holds the 3x3 patches of the style activations on a grid
    of stride >= `mrf_stride`, at most `mrf_max_patches` of them.  Blend weights do not enter that term - a patch is matched or it is not -
    except that a style image of blend weight 0 gives no patches; use_covariance does not change it.  With `swd_factor > 0` it gains
    swd_factor s, s the sliced Wasserstein term of DESIGN.md section 17 over `swd_directions` directions (0: as many as channels) drawn once
    from `swd_seed` and the layer's `swd_index`, matched over `swd_bins` bins to a target of `swd_knots` quantiles per direction;
    use_covariance does not change it.  The dynamic term gets none of these."""

    def __init__(self, strength, use_covariance=False, normalize=False, video_style_factor=0, shift_factor=0,
                 flip_factor=0, rotation_factor=0):
        super().__init__()
        self.reset_targets()
        self.strength = strength
        self.blend_weight = None
        self.video_style_factor = video_style_factor
        self.shift_factor = shift_factor
        self.flip_factor = flip_factor
        self.rotation_factor = rotation_factor
        # (not a constructor argument: the reference has none) True: a module with shift or mirror terms is evaluated by engine.StyleEngine
        # ("terms steps") instead of sending the whole network to the module path; models.py sets it from the preset
        # key `terms_engine`
        self.terms_engine = False
        # (no constructor arguments either) the feature-histogram term: models.py sets them from the preset keys of the same names
        self.hist_loss_factor = 0.0
        self.hist_loss_bins = 256
        self.hist_loss_knots = 1024
        # (nor here) the MRF patch-matching term: preset keys of the same names; models.py gives the factor to the layers of `mrf_layers`
        self.mrf_factor = 0.0
        self.mrf_stride = 2
        self.mrf_max_patches = 16384
        # (nor here) the sliced Wasserstein term: preset keys of the same names; models.py also sets the layer's index among the style layers
        self.swd_factor = 0.0
        self.swd_directions = 0
        self.swd_seed = 0
        self.swd_bins = 256
        self.swd_knots = 1024
        self.swd_index = 0
        self.gram = GramMatrix()
        self.crit = _MseFn.apply
        self.loss = 0
        self.mode = "none"
        self.use_covariance = use_covariance
        self.normalize = normalize
        self._guide = None
        self._layer_guides = {}

    def reset_targets(self):
        self.target = torch.Tensor()
        self.video_target = torch.Tensor()
        self.shift_targets_x = []  # one (C, C) target per entry of shift_target_deltas: sum of blend weight x shifted Gram along x
        self.shift_targets_y = []  # ... along y
        self.shift_target_deltas = None  # the deltas every capture pass so far produced (None: nothing captured)
        self._shift_dropped = set()  # deltas some capture pass produced and another did not
        self._shift_named = set()
        self.flip_targets = {}  # mirror kind (0 = LR, 1 = UD, 2 = point mirror) -> (C, C): sum of blend weight x mirrored Gram
        self.hist_target = None  # (C, hist_loss_knots): sum of blend weight x quantile table of the style's activation
        self.mrf_bank = None  # (S (C, Hs, Ws), origin (P,) int32, inv (P,)) on the device, built from _mrf_maps at the first evaluation
        self._mrf_maps = []  # the captured style activations (C, Hs_i, Ws_i), in capture order
        self.swd_target = None  # (D, swd_knots): sum of blend weight x quantile table of the style's projected activation
        self._swd_dirs = None  # (V (D, C), V^T (C, D)) on the device, drawn at the first capture
        self.guided_target = None  # (R, C, C): sum over the style images of blend weight x guided Gram, per region
        self.guided_weight = None  # R blend-weight sums over the style images in which the region is active
        self._guided_ready = None

    # -- spatial control (Gatys et al. 2017): None, or R <= 8 guides at image resolution, (R, H, W) device tensor with values in [0, 1].
    # In capture mode they are the guides of the style image being captured, in loss mode those of the content image
    # (optim.set_style_targets / optim.optimize set them).  The layer guides are derived once per activation shape.
    @property
    def guide(self):
        return self._guide

    @guide.setter
    def guide(self, value):
        if value is not None:
            if value.dim() != 3 or not 1 <= value.shape[0] <= 8:
                raise ValueError(f"guide: expected (R, H, W) with 1 <= R <= 8, got {tuple(value.shape)}")
            if not value.is_cuda:
                raise hip.HipError("guide: a ROCm device tensor is needed (there is no CPU path)")
        if value is not self._guide:
            self._layer_guides = {}
        self._guide = value

    def layer_guides(self, channels, hl, wl):
        key = (int(channels), int(hl), int(wl))
        if key not in self._layer_guides:
            self._layer_guides[key] = LayerGuides(self._guide, *key)
        return self._layer_guides[key]

    def guided_targets(self):
        """(T (R, C, C), has_target [R]): T_r = sum_i b_i G_r(style_i) / sum of b_i over the styles in which r is active.  A region that
        is active in no style image has no target; it is named once on stderr."""
        if self._guided_ready is None:
            has = [w > 0 for w in self.guided_weight]
            inv = torch.tensor([1.0 / w if h else 0.0 for w, h in zip(self.guided_weight, has)], dtype=torch.float32,
                               device=self.guided_target.device)
            for r, h in enumerate(has):
                if not h:
                    print(f"{getattr(self, 'name', 'StyleLoss')}: region {r} is active in no style image here: no style term for it",
                          file=sys.stderr)
            self._guided_ready = (self.guided_target * inv[:, None, None], has)
        return self._guided_ready

    def guided_loss(self, input):
        if input.shape[0] != 1:
            raise NotImplementedError("guided StyleLoss: one frame per evaluation (B = 1)")
        C, H, W = input.shape[1:]
        lg = self.layer_guides(C, H, W)
        grams = _GuidedGramFn.apply(input, lg.g, lg.scale, lg.mass, bool(self.use_covariance))
        if self.mode == "capture":
            self.loss = 0
            if self.guided_target is None:
                self.guided_target = torch.zeros_like(grams)
                self.guided_weight = [0.0] * grams.shape[0]
            elif self.guided_target.shape != grams.shape:
                raise ValueError("guided StyleLoss: every style image needs guides for the same regions")
            self.guided_target = self.guided_target + self.blend_weight * grams.detach()  # (an inactive region's matrix is zeros)
            self.guided_weight = [w + (self.blend_weight if a else 0.0) for w, a in zip(self.guided_weight, lg.active)]
            self._guided_ready = None
        if self.mode == "loss":
            if self.guided_target is None:
                raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: guided style target not captured")
            if self.guided_target.shape != grams.shape:
                raise ValueError("guided StyleLoss: content and style guides must name the same regions")
            target, has = self.guided_targets()
            for r in range(grams.shape[0]):
                if not (lg.active[r] and has[r]):
                    continue
                # the static and - with video_style_factor > 0 - the dynamic term of the unguided module, which coincide for one frame
                t = self.crit(grams[r], target[r])
                self.loss += self._accumulate(t) * self.strength
                if self.video_style_factor > 0:
                    self.loss += self.video_style_factor * self._accumulate(t) * self.strength

    def forward(self, input):
        if self.mode == "none":
            return input
        if self._guide is not None:
            if self.shift_factor > 0:
                raise NotImplementedError("StyleLoss: guides and shift_factor > 0 together are not implemented")
            if self.flip_factor > 0 or self.rotation_factor > 0:
                raise NotImplementedError("StyleLoss: guides and flip_factor / rotation_factor > 0 together are not implemented")
            if self.hist_loss_factor > 0:
                raise NotImplementedError("StyleLoss: guides and hist_loss_factor > 0 together are not implemented")
            if self.mrf_factor > 0:
                raise NotImplementedError("StyleLoss: guides and mrf_factor > 0 together are not implemented")
            if self.swd_factor > 0:
                raise NotImplementedError("StyleLoss: guides and swd_factor > 0 together are not implemented")
            self.guided_loss(input)
            return input
        self.static_loss(input)
        if self.video_style_factor > 0:
            self.dynamic_loss(input)
        return input

    def _accumulate(self, loss):
        if self.normalize:
            loss = ScaleGradients.apply(loss, self.strength)
        return loss

    def static_loss(self, input):
        frames = input.shape[0]
        for idx in range(frames):
            frame = input[idx].unsqueeze(0)
            gram = self.gram(frame, use_covariance=self.use_covariance) / frame.nelement()
            if self.mode == "capture":
                self.loss = 0
                contrib = self.blend_weight * gram.detach() / frames
                self.target = contrib if self.target.nelement() == 0 else self.target + contrib
            if self.mode == "loss":
                t = self.crit(gram, self.target)
                if self.shift_factor > 0:
                    t = self._shift_terms(frame, t)
                if self.mirror_kinds():
                    t = self._flip_terms(frame, t)
                if self.hist_loss_factor > 0:
                    t = self._hist_terms(frame, t)
                if self.mrf_factor > 0:
                    t = self._mrf_terms(frame, t)
                if self.swd_factor > 0:
                    t = self._swd_terms(frame, t)
                self.loss += self._accumulate(t) * self.strength / frames
            if self.mode == "capture" and self.shift_factor > 0:
                self._shift_capture(frame, frames)
            if self.mode == "capture" and self.mirror_kinds():
                self._flip_capture(frame, frames)
            if self.mode == "capture" and self.hist_loss_factor > 0:
                self._hist_capture(frame, frames)
            if self.mode == "capture" and self.mrf_factor > 0:
                self._mrf_capture(frame)
            if self.mode == "capture" and self.swd_factor > 0:
                self._swd_capture(frame, frames)

    # -- long-range consistency (shift_factor > 0): G_s of loss.shift_deltas(H, W) along x and y, matched like the static Gram matrix
    def _shift_grams(self, frame, deltas):
        shifts = [(axis, d) for d in deltas for axis in (0, 1)]
        return _ShiftGramFn.apply(frame, shifts, bool(self.use_covariance), None)  # rows 2 i, 2 i + 1: deltas[i] along x, y

    def _shift_capture(self, frame, frames):
        deltas = shift_deltas(frame.shape[2], frame.shape[3])
        if self.shift_target_deltas is None:
            C = frame.shape[1]
            self.shift_target_deltas = list(deltas)
            self.shift_targets_x = [torch.zeros(C, C, device=frame.device) for _ in deltas]
            self.shift_targets_y = [torch.zeros(C, C, device=frame.device) for _ in deltas]
        keep = [d for d in self.shift_target_deltas if d in deltas]
        self._shift_dropped |= (set(deltas) | set(self.shift_target_deltas)) - set(keep)
        at = [self.shift_target_deltas.index(d) for d in keep]
        self.shift_targets_x = [self.shift_targets_x[i] for i in at]
        self.shift_targets_y = [self.shift_targets_y[i] for i in at]
        self.shift_target_deltas = keep
        if keep:
            grams = self._shift_grams(frame, keep).detach()
            for i in range(len(keep)):
                self.shift_targets_x[i] = self.shift_targets_x[i] + self.blend_weight * grams[2 * i] / frames
                self.shift_targets_y[i] = self.shift_targets_y[i] + self.blend_weight * grams[2 * i + 1] / frames

    def shift_deltas_used(self, h, w):
        """The deltas of the shift terms for a working layer of h x w: those every capture pass produced and this layer has.  Any other
        delta of either side is dropped and named once on stderr."""
        if self.shift_target_deltas is None:
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: shift targets not captured")
        here = shift_deltas(h, w)
        use = [d for d in self.shift_target_deltas if d in here]
        for d in sorted((set(here) | set(self.shift_target_deltas) | self._shift_dropped) - set(use) - self._shift_named):
            self._shift_named.add(d)
            print(f"{getattr(self, 'name', 'StyleLoss')}: shift {d} is not produced by every style image and the working image here: "
                  "no shift term for it", file=sys.stderr)
        return use

    def _shift_terms(self, frame, t):
        use = self.shift_deltas_used(frame.shape[2], frame.shape[3])
        if not use:
            return t
        grams = self._shift_grams(frame, use)
        for i, d in enumerate(use):
            at = self.shift_target_deltas.index(d)
            t = t + self.shift_factor * (self.crit(grams[2 * i], self.shift_targets_x[at]) + self.crit(grams[2 * i + 1], self.shift_targets_y[at]))
        return t

    # -- symmetry (flip_factor, rotation_factor > 0): G_m of the mirrors in use, matched like the static Gram matrix
    def mirror_kinds(self):
        """The mirror kinds in use: LR and UD with flip_factor > 0, the point mirror with rotation_factor > 0."""
        return ([MIRROR_LR, MIRROR_UD] if self.flip_factor > 0 else []) + ([MIRROR_180] if self.rotation_factor > 0 else [])

    def _flip_capture(self, frame, frames):
        kinds = self.mirror_kinds()
        grams = _FlipGramFn.apply(frame, kinds, bool(self.use_covariance), None).detach()
        for i, kind in enumerate(kinds):
            contrib = self.blend_weight * grams[i] / frames
            self.flip_targets[kind] = contrib if kind not in self.flip_targets else self.flip_targets[kind] + contrib

    def _flip_terms(self, frame, t):
        kinds = self.mirror_kinds()
        missing = [k for k in kinds if k not in self.flip_targets]
        if missing:
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: mirror targets not captured (kinds {missing})")
        grams = _FlipGramFn.apply(frame, kinds, bool(self.use_covariance), None)
        for i, kind in enumerate(kinds):
            factor = self.rotation_factor if kind == MIRROR_180 else self.flip_factor
            t = t + factor * self.crit(grams[i], self.flip_targets[kind])
        return t

    # -- feature histograms (hist_loss_factor > 0): every channel matched to the blended quantile table of the style images
    def _hist_capture(self, frame, frames):
        contrib = self.blend_weight * hip.feat_hist_quantiles(frame, int(self.hist_loss_knots)) / frames
        if self.hist_target is not None and self.hist_target.shape != contrib.shape:
            raise ValueError("feature histograms: hist_loss_knots changed between two capture passes")
        self.hist_target = contrib if self.hist_target is None else self.hist_target + contrib

    def _hist_terms(self, frame, t):
        if self.hist_target is None:
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: feature-histogram target not captured")
        if tuple(self.hist_target.shape) != (frame.shape[1], int(self.hist_loss_knots)):
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: feature-histogram target of shape {tuple(self.hist_target.shape)} for "
                               f"{frame.shape[1]} channels and {int(self.hist_loss_knots)} knots: capture again")
        return t + self.hist_loss_factor * _FeatHistFn.apply(frame, self.hist_target, int(self.hist_loss_bins))

    # -- MRF patch matching (mrf_factor > 0): every 3x3 patch towards its nearest patch of the bank of all style images
    def _mrf_capture(self, frame):
        if self.blend_weight == 0:  # (an image that takes no part in the blend gives no patches)
            return
        self._mrf_maps.append(frame.detach()[0].float().contiguous().clone())
        self.mrf_bank = None

    def _mrf_build(self):
        """The bank of the captured maps: stacked along the height, zero-padded to the widest, patches on loss.mrf_grid; a patch of norm 0
        (maua_mrf_bank leaves inv = 0 for it) is not listed."""
        maps = self._mrf_maps
        C, ws = maps[0].shape[0], max(m.shape[2] for m in maps)
        if any(m.shape[0] != C for m in maps):
            raise ValueError("MRF patch matching: style activations of different channel counts")
        smap = torch.zeros(C, sum(m.shape[1] for m in maps), ws, device=maps[0].device)
        top = 0
        for m in maps:
            smap[:, top:top + m.shape[1], :m.shape[2]] = m
            top += m.shape[1]
        _, origins = mrf_grid([(m.shape[1], m.shape[2]) for m in maps], self.mrf_stride, self.mrf_max_patches)
        origin = torch.tensor(origins, dtype=torch.int32)
        _, inv = hip.mrf_bank(smap, origin)
        keep = (inv > 0).cpu()
        if not bool(keep.any()):
            raise ValueError(f"{getattr(self, 'name', 'StyleLoss')}: every style patch of the MRF bank is zero")
        if not bool(keep.all()):
            origin = origin[keep].contiguous()
        od, inv = hip.mrf_bank(smap, origin)  # (the same sums again for the patches kept: the same bits)
        self.mrf_bank = (smap, od, inv)

    def _mrf_terms(self, frame, t):
        if self.mrf_bank is None:
            if not self._mrf_maps:
                raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: MRF patch bank not captured")
            self._mrf_build()
        smap, origin, inv = self.mrf_bank
        if smap.shape[0] != frame.shape[1]:
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: MRF patch bank of {smap.shape[0]} channels for {frame.shape[1]}: "
                               "capture again")
        return t + self.mrf_factor * _MrfFn.apply(frame, smap, origin, inv)

    # -- sliced Wasserstein distance (swd_factor > 0): every projection matched to the blended quantile table of the styles' projections
    def _swd_pair(self, frame):
        """(V (D, C), V^T (C, D)) on the frame's device: loss.swd_directions of this layer, fixed until reset_targets()."""
        C = frame.shape[1]
        D = int(self.swd_directions) or C
        if self._swd_dirs is None or tuple(self._swd_dirs[0].shape) != (D, C):
            v = swd_directions(C, D, self.swd_seed, self.swd_index).to(frame.device)
            self._swd_dirs = (v, v.t().contiguous())
        return self._swd_dirs

    def _swd_capture(self, frame, frames):
        v, _ = self._swd_pair(frame)
        proj, _, _ = hip.swd_project(frame.detach().float().contiguous(), v)
        contrib = self.blend_weight * hip.feat_hist_quantiles(proj, int(self.swd_knots)) / frames
        if self.swd_target is not None and self.swd_target.shape != contrib.shape:
            raise ValueError("sliced Wasserstein distance: swd_directions or swd_knots changed between two capture passes")
        self.swd_target = contrib if self.swd_target is None else self.swd_target + contrib

    def _swd_terms(self, frame, t):
        if self.swd_target is None:
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: sliced Wasserstein target not captured")
        D = int(self.swd_directions) or frame.shape[1]
        if tuple(self.swd_target.shape) != (D, int(self.swd_knots)):
            raise RuntimeError(f"{getattr(self, 'name', 'StyleLoss')}: sliced Wasserstein target of shape {tuple(self.swd_target.shape)} for "
                               f"{D} directions and {int(self.swd_knots)} knots: capture again")
        v, vt = self._swd_pair(frame)
        return t + self.swd_factor * _SwdFn.apply(frame, v, vt, self.swd_target, int(self.swd_bins))

    def dynamic_loss(self, input):
        rows = input.shape[0] * input.shape[1]
        if self.video_target.nelement() != 0 and rows != self.video_target.shape[0]:
            return  # image styles are ignored by the dynamic term when shapes differ
        gram = self.gram(input, use_covariance=self.use_covariance) / input.nelement()
        if self.mode == "capture":
            self.loss = 0
            contrib = self.blend_weight * gram.detach()
            self.video_target = contrib if self.video_target.nelement() == 0 else self.video_target + contrib
        if self.mode == "loss":
            loss = self._accumulate(self.crit(gram, self.video_target))
            self.loss += self.video_style_factor * loss * self.strength / input.shape[0]


class TVLoss(nn.Module):
    """Anisotropic (L1) total variation of the image itself (reference loss.py:224-233); always active."""

    def __init__(self, strength):
        super().__init__()
        self.strength = strength

    def forward(self, input):
        self.loss = self.strength * _TVFn.apply(input)
        return input
