"""The optimisation core with the reference's entry points (reference optim.py).

`optimize(content, styles, init, num_iters, args, net=None, losses=None)` keeps the reference's contract
(optim.py:111-255): per-size model selection through the scaling table, target capture, L-BFGS or Adam on
the pixels, CPU fp32 result of init's shape.  What changed is where the loop runs: the image, the network,
every activation, the L-BFGS history and all scalars live on the MI355X; one iteration is a fixed chain of
libmaua_hip kernels (engine.StyleEngine for the function evaluation, hip.LbfgsState / hip.adam_step for the
update) with no host synchronisation - the reference's per-module `.item()` reads (optim.py:210) and
torch.optim.LBFGS's four host round trips per iteration are gone.  The loss is read back only when
`--print_iter` fires.
"""
import json
import math
import os
import sys

import numpy as np
import torch as th
import tqdm

import config as config_mod
import engine as engine_mod
import hip
import loss as loss_mod
import plan
import models
from utils import limit_host_threads, wrapping_slice

PBAR = tqdm.tqdm(file=sys.stdout, smoothing=0.1, disable=not sys.stdout.isatty())


def _describe(text, args):
    if not args.verbose:
        PBAR.set_description(text)


def _device_image(image, args):
    return image.to(device="cuda", dtype=th.float32).contiguous()


def _device_guide(guide, image):
    """(R,H,W) guides of `image` (values in [0, 1], at its resolution) as a device tensor."""
    if guide.dim() != 3 or tuple(guide.shape[1:]) != tuple(image.shape[-2:]):
        raise ValueError(f"guides of shape {tuple(guide.shape)} for an image of {tuple(image.shape[-2:])}: expected (R, H, W) at its size")
    return guide.to(device="cuda", dtype=th.float32).contiguous()


def _guided(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) carry guides?  Such a network runs on the module path unless the
    planner field guided_engine is on."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(getattr(m, "guide", None) is not None for m in mods)


def _shifted(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) have shift_factor > 0?  Such a network runs on the module path."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(isinstance(m, loss_mod.StyleLoss) and m.shift_factor > 0 for m in mods)


def _mirrored(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) have flip_factor > 0 or rotation_factor > 0?  Such a network runs on
    the module path, like a shifted one."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(isinstance(m, loss_mod.StyleLoss) and bool(m.mirror_kinds()) for m in mods)


def _histogrammed(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) have hist_loss_factor > 0?  Such a network runs on the module path,
    whatever `terms_engine` says: the fused engine has no feature-histogram step."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(isinstance(m, loss_mod.StyleLoss) and getattr(m, "hist_loss_factor", 0) > 0 for m in mods)


def _patch_matched(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) have mrf_factor > 0?  Such a network runs on the module path,
    whatever `terms_engine` says: the fused engine has no MRF patch-matching step."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(isinstance(m, loss_mod.StyleLoss) and getattr(m, "mrf_factor", 0) > 0 for m in mods)


def _sliced(net_or_losses):
    """Does a style module of the network (or of a list of loss modules) have swd_factor > 0?  Such a network runs on the module path,
    whatever `terms_engine` says: the fused engine has no sliced Wasserstein step."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    return any(isinstance(m, loss_mod.StyleLoss) and getattr(m, "swd_factor", 0) > 0 for m in mods)


def _terms_on_module_path(net_or_losses):
    """The reason a shifted, mirrored or histogram-matched network stays on the module path, or None: a style module with
    hist_loss_factor > 0, or one with shift_factor > 0 or a mirror in use whose `terms_engine` is off (the default).  With it on the fused
    engine evaluates the shift and mirror terms (engine.py, "terms steps")."""
    mods = getattr(net_or_losses, "style_losses", net_or_losses)
    if _histogrammed(mods):
        return "feature-histogram StyleLoss runs on the module path"
    if _patch_matched(mods):
        return "MRF patch-matching StyleLoss runs on the module path"
    if _sliced(mods):
        return "sliced-Wasserstein StyleLoss runs on the module path"
    style = [m for m in mods if isinstance(m, loss_mod.StyleLoss) and not getattr(m, "terms_engine", False)]
    if _shifted(style):
        return "shifted StyleLoss runs on the module path"
    if _mirrored(style):
        return "mirrored StyleLoss runs on the module path"
    return None


def _style_targets_missing(net):
    """A style module without its target - or, with shift_factor > 0, without its shift targets, or with a mirror in use without that
    mirror's target, or with hist_loss_factor > 0 or swd_factor > 0 without its quantile table (the factor was set after the capture)."""
    return any(m.target.nelement() == 0 or (m.shift_factor > 0 and m.shift_target_deltas is None)
               or any(k not in m.flip_targets for k in m.mirror_kinds())
               or (getattr(m, "hist_loss_factor", 0) > 0 and getattr(m, "hist_target", None) is None)
               or (getattr(m, "mrf_factor", 0) > 0 and getattr(m, "mrf_bank", None) is None and not getattr(m, "_mrf_maps", None))
               or (getattr(m, "swd_factor", 0) > 0 and getattr(m, "swd_target", None) is None)
               for m in net.style_losses)


def _engine_of(net):
    """The fused engine of a loss network (built once per network; None when its module layout is not covered)."""
    if _guided(net) and not plan.on("guided_engine"):
        return None  # (not remembered: the same network without guides takes the engine again)
    if _terms_on_module_path(net) is not None:
        # (not remembered either: the same network with shift_factor, flip_factor and rotation_factor back at 0 - or with `terms_engine`
        #  set on its style modules - takes the engine again)
        return None
    eng = getattr(net, "_maua_engine", None)
    if eng is None and not getattr(net, "_maua_engine_refused", False):
        if not all(hasattr(net, a) for a in ("content_losses", "style_losses", "tv_losses", "temporal_losses")):
            net._maua_engine_refused = True  # not assembled by models.load_model: module path
            return None
        try:
            eng = engine_mod.StyleEngine(net, net.content_losses + net.style_losses + net.tv_losses + net.temporal_losses)
            net._maua_engine = eng
        except engine_mod.UnsupportedNet:  # nothing else: a bug inside the engine must not silently demote the run
            net._maua_engine_refused = True
    return eng


def set_content_targets(net, content_image, args):
    """One forward pass with the content modules in 'capture' mode (reference optim.py:22-32)."""
    _describe("Capturing content targets...", args)
    image = _device_image(content_image, args)
    eng = _engine_of(net)
    if eng is not None and (image.shape[0] == 1 or eng.independent):
        try:
            eng.capture_content(image)
            return
        except engine_mod.UnsupportedNet:
            pass
    for mod in net.content_losses:
        mod.mode = "capture"
    with th.no_grad():
        net(image)
    for mod in net.content_losses:
        mod.mode = "none"


def set_temporal_targets(net, warp_image, warp_weights=None, args=None):
    """Capture the warped previous frame as pixel-level target, optionally weighted (reference optim.py:35-47)."""
    _describe("Capturing temporal targets...", args)
    for mod in net.temporal_losses:
        mod.mode = "capture"
        if warp_weights is not None:
            mod.weights = _device_image(warp_weights, args)
    with th.no_grad():
        net(_device_image(warp_image, args))
    for mod in net.temporal_losses:
        mod.mode = "none"


def set_style_targets(net, style_images, args, style_guides=None):
    """Accumulate blend-weighted Gram targets over the style images (reference optim.py:50-66).  `style_guides`: one (R,H_i,W_i) guide
    tensor per style image - each is set on the style modules before that image's capture pass (guided targets, loss.StyleLoss)."""
    _describe("Capturing style targets...", args)
    if style_guides is not None and len(style_guides) != len(style_images):
        raise ValueError(f"{len(style_guides)} style guides for {len(style_images)} style images")
    for mod in net.style_losses:
        mod.reset_targets()
        mod.mode = "capture"
    for i, image in enumerate(style_images):
        for mod in net.style_losses:
            mod.blend_weight = args.style_blend_weights[i]
            if style_guides is not None:
                mod.guide = _device_guide(style_guides[i], image)
        with th.no_grad():
            net(_device_image(image, args))
    for mod in net.style_losses:
        mod.mode = "none"


def set_style_video_targets(net, style_videos, args):
    """Style targets averaged over every window of `gram_frame_window` consecutive frames of each style video
    (reference optim.py:69-90): the per-frame Gram target and, through StyleLoss.dynamic_loss, the cross-frame
    (B*C) x (B*C) one.  The blend weight is divided by the number of windows, as the reference does."""
    _describe("Capturing style video targets...", args)
    window = int(args.gram_frame_window)
    for mod in net.style_losses:
        mod.reset_targets()
        mod.mode = "capture"
    for i, video in enumerate(style_videos):
        n_windows = max(len(video) - window + 1, 1)
        for mod in net.style_losses:
            mod.blend_weight = args.style_blend_weights[i] / n_windows
        for start in range(n_windows):
            with th.no_grad():
                net(_device_image(video[start:start + window], args))
    for mod in net.style_losses:
        mod.mode = "none"


def set_model_args(args, current_size):
    """Copy onto `args` every key of the first scaling-table entry whose size bound covers `current_size` and
    that does not need more GPUs than --gpu lists (reference optim.py:93-108).  Like the reference, when no
    entry qualifies the LAST entry is applied after a warning."""
    with open(config_mod._resolve(args.scaling_args), "r") as f:
        scaling = json.load(f)
    found, params = False, {}
    for size, params in scaling.items():
        if int(size) < current_size:
            continue
        if len(args.gpu.split(",")) < len(params["gpu"].split(",")):
            continue
        found = True
        break
    if not found:
        print("Warning: no model configuration found for this size, out of memory error is likely...")
    for key, value in params.items():
        args.__dict__[key] = value


def lbfgs_moves(num_iters):
    """Number of (evaluate, move) pairs torch.optim.LBFGS performs under the reference's driver
    (`LBFGS(max_iter=N)`, max_eval = 5N//4, `while i[0] <= 1: step(feval)`, optim.py:180-191, 240-241):
    N >= 4 -> N; N in {2, 3} stop one move early on max_eval; N = 1 runs step() twice."""
    if num_iters <= 0:
        return 0
    if num_iters == 1:
        return 2
    if num_iters in (2, 3):
        return num_iters - 1
    return num_iters


GRAPH_MIN_ITERS = 128
GRAPH_MIN_ITERS_REPEATED = 20  # ... for calls the caller announces it will repeat on the same network and shapes (vid_img's frame batches)


class PixelOptimizer:
    """The iteration loop for one image: fused feval + device-side optimizer step."""

    def __init__(self, net, losses, init, args, planned_iters=None, grad_hook=None, independent=False, batch_hint=1, repeated=False):
        """`independent`: `init` holds B separate single-frame problems (vid_img's frames without optical flow) that are
        evaluated together - one L-BFGS state (or Adam moment pair) per frame, the single-frame loss arithmetic per frame.
        `repeated`: the caller will run more problems of this shape on this network (vid_img: one call per frame batch and pass):
        the captured iteration is kept with its image buffer and optimiser states (a "bundle" on the engine) and the next call
        replays it from its first iteration on - content / temporal targets are rewritten in place, so the graph stays valid."""
        self.args = args
        self.independent = bool(independent) and init.shape[0] > 1
        self.grad_hook = grad_hook  # in-place edit of the gradient before the optimiser sees it (img_vid's overlap masking)
        try:
            # (also on the L-BFGS bundle path below: no engine, no bundle, no captured graph - unless the planner field guided_engine is on)
            if _guided(losses) and not plan.on("guided_engine"):
                raise engine_mod.UnsupportedNet("guided StyleLoss runs on the module path")
            if _terms_on_module_path(losses) is not None:  # (shift / mirror terms whose module has `terms_engine` off)
                raise engine_mod.UnsupportedNet(_terms_on_module_path(losses))
            self.engine = getattr(net, "_maua_engine", None) or engine_mod.StyleEngine(net, losses)
            net._maua_engine = self.engine
        except engine_mod.UnsupportedNet:
            self.engine = None
        self.net, self.losses = net, losses
        self.x = _device_image(init, args).clone()
        self.kind = args.optimizer
        self.step_count = 0
        self.batch_hint = max(1, int(batch_hint))
        if self.engine is not None:
            self.engine.independent, self.engine.batch_hint = self.independent, self.batch_hint
        elif self.independent:
            raise engine_mod.UnsupportedNet("independent frame batches need the fused engine")
        # A bundle of an earlier call on this network: same shapes, same optimiser parameters, and nothing the captured graph
        # baked in has moved since (engine buffers: alloc_epoch; targets / weights / coefficients: _graph_key)
        self._bundle_key, bundle = None, None
        if self.engine is not None and self.kind == "lbfgs" and grad_hook is None and plan.on("graph_bundles"):
            self._bundle_key = ("lbfgs", tuple(self.x.shape), str(self.x.device), str(self.x.dtype), self.independent, self.batch_hint,
                                int(args.lbfgs_num_correction), float(args.lbfgs_tolerance_change), float(args.lbfgs_tolerance_grad))
            try:
                self.engine._prepare(self.x)  # (allocates for this shape if the engine last served another one: a new epoch)
            except engine_mod.UnsupportedNet:  # (a guided or terms layer the engine does not take here: module path)
                if self.independent:
                    raise
                self.engine, self._bundle_key = None, None
        if self._bundle_key is not None:
            bundle = self.engine.iter_graphs.get(self._bundle_key)
            if bundle is not None and (bundle["epoch"] != self.engine.alloc_epoch or bundle["graph_key"] != self.engine._graph_key()):
                bundle = None
                del self.engine.iter_graphs[self._bundle_key]
            # (a bundle's image and L-BFGS states are ITS buffers: an optimiser that is still alive on it keeps it - a second one with
            #  the same key works on fresh buffers and captures its own graph instead of aliasing the first one's state)
            owner = bundle.get("owner") if bundle is not None else None
            if owner is not None and owner() is not None and owner() is not self:
                bundle = None
            elif bundle is not None:
                import weakref
                bundle["owner"] = weakref.ref(self)
        if bundle is not None:
            bundle["x"].copy_(self.x)
            self.x = bundle["x"]
        self.frames = [self.x[b] for b in range(self.x.shape[0])] if self.independent else [self.x]
        if self.kind == "lbfgs":
            if bundle is not None:
                self.states = bundle["states"]
                for st in self.states:
                    st.reset()
            else:
                self.states = [hip.LbfgsState(f.numel(), int(args.lbfgs_num_correction), self.x.device) for f in self.frames]
            self.state = self.states[0]
        elif self.kind == "adam":
            self.m, self.v = th.zeros_like(self.x), th.zeros_like(self.x)
        else:
            raise ValueError(f"unknown optimizer {self.kind}")
        # The whole iteration (25+ convolutions, Grams, losses, the optimiser sweeps: ~120 launches, every scalar on the
        # device) is replayed from one captured hipGraph.  MAUA_HIP_GRAPH=0 or an attached engine timer runs it eagerly.
        # Capturing costs ~30 ms (torch synchronises, collects garbage and empties its cache around a capture) and a replay
        # saves ~0.25 ms of launch gaps per iteration: runs shorter than GRAPH_MIN_ITERS (vid_img's 25-50 iterations per
        # call) launch eagerly.
        hg = getattr(args, "hip_graph", None)
        if hg is None:
            enough = planned_iters is None or planned_iters >= (GRAPH_MIN_ITERS_REPEATED if repeated and self._bundle_key else GRAPH_MIN_ITERS)
            hg = plan.on("hip_graph") and (enough or bundle is not None)
        self.use_graph = bool(hg)
        self._graph = bundle["graph"] if (bundle is not None and self.use_graph) else None
        self._keep_bundle = bool(repeated) and self._bundle_key is not None
        self.owns_x = bundle is None and not self._keep_bundle  # (else `x` lives on in the bundle: callers get a copy)

    def feval(self):
        """(loss slots, total, gradient) at the current image - device tensors, no sync."""
        if self.engine is not None:
            self.engine.independent, self.engine.batch_hint = self.independent, self.batch_hint
            try:
                return self.engine.feval(self.x, capture=self.use_graph and self.kind != "lbfgs" and self.engine.timer is None)
            except engine_mod.UnsupportedNet:
                self.engine = None
        return self._feval_modules()

    def _feval_modules(self):
        """Module-by-module evaluation with autograd (still HIP kernels): covers layouts outside the fused plan,
        e.g. the weighted temporal ContentLoss."""
        x = self.x.detach().requires_grad_(True)
        self.net(x)
        total = 0
        slots = th.zeros(max(len(self.losses), 1), device=x.device)
        for idx, mod in enumerate(self.losses):
            if isinstance(mod.loss, int) and mod.loss == 0:
                continue
            slots[idx] = mod.loss.detach()
            total = total + mod.loss
        total.backward()
        for mod in self.losses:
            mod.loss = 0
        return slots, total.detach().reshape(1), x.grad.contiguous()

    def _lbfgs_move(self, grad, total):
        """One L-BFGS update per frame (a single one unless `independent`): device-side, no sync."""
        a = self.args
        eng = self.engine if self.independent else None
        if eng is not None:
            eng.fork()  # each frame's five kernels (two bandwidth-bound sweeps around a one-wave serial chain) on its own stream
        for b, (st, xf) in enumerate(zip(self.states, self.frames)):
            gb = grad[b] if self.independent else grad
            lb = None
            if th.is_tensor(total) and total.is_cuda:
                lb = total[b:b + 1] if self.independent else total
            if eng is not None:
                ctx, _ = eng.frame_stream(b)
                with ctx:
                    st.iterate(xf, gb, 1.0, float(a.lbfgs_tolerance_change), float(a.lbfgs_tolerance_grad), lb)
            else:
                st.iterate(xf, gb, 1.0, float(a.lbfgs_tolerance_change), float(a.lbfgs_tolerance_grad), lb)
        if eng is not None:
            eng.join()

    def stopped(self):
        """Every frame's L-BFGS has hit one of its stop tests (host sync; called every 25 iterations)."""
        return self.kind == "lbfgs" and all(st.status()["stopped"] for st in self.states)

    def _step_lbfgs_graph(self):
        """feval + L-BFGS update as one graph replay; the first call runs eagerly (a real iteration) and captures."""
        if self._graph is not None:
            self._graph.replay()
            self.step_count += 1
            return self.engine.slots, self.engine.total
        slots, total, grad = self.engine.feval(self.x)
        if self.grad_hook is not None:
            self.grad_hook(grad)
        self._lbfgs_move(grad, total)
        self.step_count += 1
        th.cuda.synchronize()
        graph = th.cuda.CUDAGraph()
        with th.cuda.graph(graph):
            self.engine._run(self.x)
            if self.grad_hook is not None:
                self.grad_hook(self.engine.gbuf[0])
            self._lbfgs_move(self.engine.gbuf[0], self.engine.total)
        self._graph = graph
        if self._keep_bundle:
            import weakref
            self.engine.iter_graphs[self._bundle_key] = {"graph": graph, "x": self.x, "states": self.states, "epoch": self.engine.alloc_epoch,
                                                         "graph_key": self.engine._graph_key(), "owner": weakref.ref(self)}
        return slots, total

    def step(self):
        """One iteration: evaluate, then move."""
        if self.use_graph and self.kind == "lbfgs" and self.engine is not None and self.engine.timer is None:
            try:
                return self._step_lbfgs_graph()
            except engine_mod.UnsupportedNet:
                self.engine = None
        slots, total, grad = self.feval()
        if self.grad_hook is not None:
            self.grad_hook(grad)
        self.step_count += 1
        a = self.args
        if self.kind == "lbfgs":
            self._lbfgs_move(grad, total)
        else:
            hip.adam_step(self.x, grad, self.m, self.v, self.step_count, float(a.learning_rate))
        return slots, total


def _run_iterations(opt, num_iters, args, save_offset=0, save_total=None):
    """The reference's `while i[0] <= iters: optimizer.step(feval)` loop (optim.py:196-241) on a PixelOptimizer."""
    if args.optimizer == "lbfgs":
        _describe("Running optimization with L-BFGS", args)
        steps = lbfgs_moves(num_iters)
    else:
        _describe("Running optimization with ADAM", args)
        steps = num_iters + 1  # `while i[0] <= iters` with i starting at 0 (optim.py:240)
    for i in range(1, steps + 1):
        if args.save_iter > 0 and (i % args.save_iter == 0 or i == num_iters):
            # the reference saves inside evaluation i (optim.py:230-236): the image BEFORE the move of iteration i
            import load
            last = save_offset + i == (save_total if save_total is not None else num_iters)
            load.save_tensor_to_file(opt.x.detach().cpu(), args, None if last else save_offset + i, opt.x.size(3))
        slots, total = opt.step()
        if not args.verbose and not (args.optimizer == "adam" and i == 1):
            PBAR.update(1)
        if args.print_iter > 0 and i % args.print_iter == 0 and args.verbose:
            print(f"Iteration {i} / {args.num_iters}, Loss: {float(total.sum())}")
        if args.optimizer == "lbfgs" and i % 25 == 0 and opt.stopped():
            break  # g.d > -tolerance_change (or another stop test): the reference breaks out of LBFGS.step here


def video_windows(init, styles, window):
    """Start frames of the optimisation windows over the pastiche and of the matching windows over every style video
    (reference optim.py:113-123): ceil(T / window) + 1 starts spaced linearly over each sequence's own length."""
    num_windows = math.ceil(init.shape[0] / window)
    seqs = [init] + list(styles)
    framestep = np.array([seq.shape[0] - window / 2 for seq in seqs]) / num_windows
    return [[math.ceil(framestep[k] * n) for n in range(num_windows + 1)] if seq.shape[0] != 1 else [0] * (num_windows + 1)
            for k, seq in enumerate(seqs)]


def _optimize_video(content, styles, init, num_iters, args, net=None, losses=None, keep_on_device=False):
    """optim.optimize for transfer types with '_vid' (reference optim.py:111-255): the pastiche is a clip, optimised
    `gram_frame_window` frames at a time (one batch of B frames through the network: per-frame static style terms and
    the cross-frame dynamic Gram term of StyleLoss.dynamic_loss, loss.py:164-181).  Windows overlap; frames already
    styled by the previous window (and, at the wrap-around, by the first) get their gradient zeroed, and every window is
    written back into the clip through the same wrapping index.  The window of B frames runs through
    the fused plan (engine.StyleEngine with B > 1: per-frame static Gram terms plus one (B C) x (B C) dynamic Gram).
    `keep_on_device=True` with a device `init`: the clip, the window gather and the write-back stay where `init` lives (no host copy
    per window) and the device clip is returned; otherwise the clip is a CPU tensor, as in the reference."""
    limit_host_threads()
    on_device = bool(keep_on_device) and init.is_cuda
    window = int(args.gram_frame_window)
    windows = video_windows(init, styles, window)
    if net is None or losses is None:
        set_model_args(args, max(*init.shape))
        net, losses = models.load_model(args)
    if not args.verbose:
        PBAR.reset()
        PBAR.total = len(windows[0]) * num_iters
        PBAR.refresh()
    set_content_targets(net, content, args)
    if args.avg_frame_window == -1:  # one set of targets from the whole style videos
        set_style_video_targets(net, styles, args)
        for mod in losses:
            mod.mode = "loss"

    output = init.clone()
    for w, window_start in enumerate(windows[0]):
        front_overlap = windows[0][w - 1] + window - window_start
        end_overlap = (window_start + window) % output.shape[0] if window_start + window >= output.shape[0] else 0
        index = wrapping_slice(output, window_start, window, return_indices=True)
        if args.avg_frame_window != -1:  # targets from the stretch of every style video that accompanies this window
            current_styles = [wrapping_slice(style, windows[k + 1][w], args.avg_frame_window) for k, style in enumerate(styles)]
            set_style_video_targets(net, current_styles, args)
            for mod in losses:
                mod.mode = "loss"
        if w == 0 and args.normalize_weights:  # once, strengths are not reset (optim.py:176-178)
            for mod in net.content_losses + net.style_losses + net.temporal_losses:
                mod.strength = mod.strength / max(mod.target.size())

        def mask_overlap(grad, w=w, front=front_overlap, end=end_overlap):
            if w != 0:  # same slices as the reference (optim.py:218-221), Python semantics included
                grad[:front] = 0
                if end > 0:
                    grad[-end:] = 0

        if on_device:
            index = index.to(output.device)
        opt = PixelOptimizer(net, losses, output[index], args, planned_iters=num_iters, grad_hook=mask_overlap)
        _run_iterations(opt, num_iters, args, save_offset=w * num_iters, save_total=len(windows[0]) * num_iters)
        if on_device:
            output[index] = opt.x.detach().to(output.dtype)
        else:
            output[index] = opt.x.detach().cpu().to(output.dtype)
        del opt
    for mod in losses:
        mod.loss = 0
    return output


def optimize_frames(contents, styles, inits, num_iters, args, net, losses, planned_frames=None):
    """B independent calls of `optimize` (same network, same style images, one content frame and one initial image each -
    the frames of vid_img without optical flow, reference style.py:192-290) evaluated as ONE batch: the convolutions and
    pools run on all B frames at once, every frame keeps its own loss terms and its own optimiser state, and each frame's
    result is bit-identical to what a separate call gives.  Tensors may live on the device; returns the (B,3,H,W) device
    tensor.  `planned_frames`: how many frames the JOB evaluates per launch (default: this call's B); the convolutions' split-K
    policy is fixed by it, so calls with the same value give the same bits for a frame whatever their own B (vid_img's short
    last batch, or its frame-by-frame debugging mode)."""
    limit_host_threads()
    if contents.shape[0] != inits.shape[0]:
        raise ValueError("one content frame per initial image")
    eng = _engine_of(net)
    if eng is None:
        raise engine_mod.UnsupportedNet("frame batches need a network the fused engine covers")
    if contents.shape[0] > 1 and (_shifted(net) or _mirrored(net)):  # (`terms_engine` on: the engine takes those terms for one frame only)
        raise engine_mod.UnsupportedNet("shifted / mirrored StyleLoss on the engine: one frame per evaluation (B = 1)")
    hint = int(planned_frames) if planned_frames else int(contents.shape[0])
    eng.independent, eng.batch_hint = contents.shape[0] > 1, hint
    if not args.verbose:
        PBAR.reset()
        PBAR.total = num_iters
        PBAR.refresh()
    set_content_targets(net, contents, args)
    key = (tuple((s.data_ptr(), tuple(s.shape), s._version) for s in styles), tuple(args.style_blend_weights))
    if getattr(net, "_maua_style_key", None) != key or _style_targets_missing(net):
        set_style_targets(net, styles, args)
        net._maua_style_key = key
        net._maua_style_refs = list(styles)
    for mod in losses:
        mod.mode = "loss"
    if args.normalize_weights:
        for mod in net.content_losses + net.style_losses + net.temporal_losses:
            mod.strength = mod.strength / max(mod.target.size())
    opt = PixelOptimizer(net, losses, inits, args, planned_iters=num_iters, independent=True, batch_hint=hint,
                         repeated=not args.normalize_weights)  # (compounding strengths change the graph's coefficients every call)
    _run_iterations(opt, num_iters, args)
    for mod in losses:
        mod.loss = 0
    return opt.x.detach() if opt.owns_x else opt.x.detach().clone()


def optimize(content, styles, init, num_iters, args, net=None, losses=None, keep_on_device=False, guides=None):
    """Optimise `init` towards `content` / `styles`; returns a CPU fp32 tensor shaped like `init` (the reference's contract,
    optim.py:249).  Inputs may already live on the device; `keep_on_device=True` (the workflow drivers of style.py) returns
    the device tensor instead, so that colour matching, rescaling and the next scale run without a host round trip.
    `guides` = (content guides (R,H,W), [style guides (R,H_i,W_i) per style image]), values in [0, 1] at each image's resolution, 1 <= R
    <= 8: spatial control - every style layer matches one Gram matrix per region (loss.StyleLoss.guide) instead of one of the whole plane.
    One frame only; the evaluation runs module by module (autograd over the HIP kernels) unless the planner field guided_engine is on:
    then the guided layers run inside the fused engine and its captured graph."""
    if guides is not None and ("_vid" in args.transfer_type or init.shape[0] != 1):
        raise NotImplementedError("guides (spatial control of the style loss) are implemented for one image per call (img_img), "
                                  "not for clips or frame batches")
    if "_vid" in args.transfer_type:
        return _optimize_video(content, styles, init, num_iters, args, net, losses, keep_on_device=keep_on_device)
    limit_host_threads()
    if init.shape[0] != 1:
        raise NotImplementedError("one frame per call (the reference's img_img / vid_img call pattern)")

    if net is None or losses is None:
        set_model_args(args, max(*init.shape))
        net, losses = models.load_model(args)

    if not args.verbose:
        PBAR.reset()
        PBAR.total = num_iters
        PBAR.refresh()

    eng = _engine_of(net)
    if eng is not None:
        eng.independent, eng.batch_hint = False, 1
    hip.set_split_batch_hint(1)
    set_content_targets(net, content, args)
    # Style targets depend only on the style images and blend weights.  The reference recaptures them on every call
    # (style.py:178 keeps the hoisting commented out); the result is identical, so a prebuilt net that is called again
    # with the same style tensors (vid_img: once per frame) keeps its targets.
    key = (tuple((s.data_ptr(), tuple(s.shape), s._version) for s in styles), tuple(args.style_blend_weights))
    if guides is not None:
        content_guide, style_guides = guides
        if len(net.style_losses) == 0:
            raise ValueError("guides need at least one style layer")
        set_style_targets(net, styles, args, style_guides=list(style_guides))
        net._maua_style_key = None  # (guided targets: the next call captures again)
        guide = _device_guide(content_guide, init)
        for mod in net.style_losses:
            mod.guide = guide
    else:
        if _guided(net):  # a network an earlier call guided: back to whole-plane targets
            for mod in net.style_losses:
                mod.guide = None
            net._maua_style_key = None
        if getattr(net, "_maua_style_key", None) != key or _style_targets_missing(net):
            set_style_targets(net, styles, args)
            net._maua_style_key = key
            net._maua_style_refs = list(styles)  # keep the tensors alive so that data_ptr stays unique
    for mod in losses:
        mod.mode = "loss"

    if args.normalize_weights:  # once per call, strengths are not reset (optim.py:176-178)
        for mod in net.content_losses + net.style_losses + net.temporal_losses:
            mod.strength = mod.strength / loss_mod.target_dim(mod)

    opt = PixelOptimizer(net, losses, init, args, planned_iters=num_iters, repeated=bool(getattr(args, "_maua_repeated_calls", False)))
    _run_iterations(opt, num_iters, args)

    for mod in losses:
        mod.loss = 0
    if not keep_on_device:
        return opt.x.detach().cpu()
    return opt.x.detach() if opt.owns_x else opt.x.detach().clone()
