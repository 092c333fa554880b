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
    """(B*C) x (B*C) Gram matrix of a feature batch, or its covariance form (reference loss.py:67-91).  The
    shift/flip arguments exist in the reference's signature but its code always ends with y = x (and its
    `::-1` slices are illegal in torch), so they are accepted and have no effect here either."""

    def forward(self, x, shift_x=0, shift_y=0, shift_t=0, flip_h=False, flip_v=False, use_covariance=False):
        return _GramFn.apply(x, use_covariance)


class StyleLoss(nn.Module):
    """Gram-matrix MSE against blended style targets (reference loss.py:94-186): a per-frame 'static' term
    and, when video_style_factor > 0 (the default, 100), a whole-batch 'dynamic' term."""

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
        self.shift_targets_x = []
        self.shift_targets_y = []
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
                self.loss += self._accumulate(self.crit(gram, self.target)) * self.strength / frames

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
