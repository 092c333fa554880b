"""Optical flow for vid_img's temporally consistent path (reference flow.py and load.process_content_video, load.py:141-188).

The reference estimates flow with four downloaded networks (unflow, pwc, spynet, liteflownet: empty submodules there, weights
from the internet).  This module offers a weight-free estimator instead, selected with `--flow_models tvl1`: coarse-to-fine
TV-L1 on the MI355X (csrc/flow.hip; DESIGN.md "Optical flow").  It writes the flow cache in the reference's layout
(`<output_dir>/<clip>_<styles>/flow/{forward,backward}_<a>_<b>.{flo,png}`), which style._vid_img_flow consumes unchanged.

    estimate_tvl1(img1, img2)       (h, w, 2) float32 flow (u, v) in pixels: img1(x) ~ img2(x + flow(x))
    check_consistency(f1, f2)       the reliability PNG's bytes, (1 - r) * 255, r = the reference's mask (computed on the device)
    flow_to_image(flow)             Middlebury colour coding (host numpy), for --no_check_occlusion
    get_flow_model(args)            "tvl1" -> the estimator; anything else needs downloaded weights and is refused
    write_flow_cache(model, args)   the reference's loop over frame pairs (wrap-around pair last -> first, resume)
"""
import os

import numpy as np
import torch as th
from PIL import Image

import hip
import load
from utils import name

TVL1_LEVELS = 5
TVL1_WARPS = 5
TVL1_ITERS = 100
# TV-L1 iterations per launch of the temporally blocked kernel (0 = the single-step kernel; same bits either way).  Chosen from
# tools/bench_flow.py on one MI355X (profiles/flow_bench.md).
TVL1_BLOCK_K = 4


def flow_model_names(args):
    return [m.strip() for m in str(getattr(args, "flow_models", "")).split(",") if m.strip()]


def uses_tvl1(args):
    return "tvl1" in flow_model_names(args)


def _device_frame(img):
    a = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected an (h, w, 3) uint8 RGB frame, got shape {a.shape}")
    return th.from_numpy(a).cuda()


def estimate_tvl1(img1_u8, img2_u8, levels=TVL1_LEVELS, warps=TVL1_WARPS, iters=TVL1_ITERS, block_k=TVL1_BLOCK_K):
    """Flow from img1 to img2 ((h, w, 3) uint8 RGB arrays): (h, w, 2) float32, channels (u, v) in pixels, img1(x) ~ img2(x + flow(x)).
    `levels` is an upper bound (the pyramid stops before the shorter side drops below 16); warps x iters per level are fixed."""
    if np.shape(img1_u8) != np.shape(img2_u8):
        raise ValueError(f"frame shapes differ: {np.shape(img1_u8)} vs {np.shape(img2_u8)}")
    a, b = _device_frame(img1_u8), _device_frame(img2_u8)
    h, w = a.shape[:2]
    flow = hip.flow_tvl1(a, b, hip.flow_levels(h, w, levels), warps, iters, block_k)
    return flow.permute(1, 2, 0).contiguous().cpu().numpy()


def _planes(flow):
    f = np.asarray(flow, dtype=np.float32)
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError(f"expected an (h, w, 2) flow field, got shape {f.shape}")
    return th.from_numpy(np.ascontiguousarray(f.transpose(2, 0, 1))).cuda()


def check_consistency(flow1, flow2):
    """Reliability of flow1 given the reverse flow2 (reference flow.py:77-137), as the uint8 image the reference saves:
    (1 - r) * 255 with r in {0, 1}.  r = 1 where the 41 x 41 window around a pixel is all 'reliable' (round trip consistent,
    inside the frame, no motion edge): what the reference's integer Gaussian blur + clip computes.  So 0 marks reliable pixels
    and 255 the rest - and load.reliable_flow_weighting, like the reference's, weights the temporal loss by these bytes / 255."""
    h, w = np.shape(flow1)[:2]
    if np.shape(flow1) != np.shape(flow2) or h < 2 or w < 2:
        raise ValueError(f"flows of shape {np.shape(flow1)} / {np.shape(flow2)}: need equal (h, w, 2) with h, w >= 2")
    return hip.flow_consistency(_planes(flow1), _planes(flow2)).cpu().numpy()


def _color_wheel():
    """The 55 colours of the Middlebury flow colour code: red-yellow 15, yellow-green 6, green-cyan 4, cyan-blue 11, blue-magenta 13,
    magenta-red 6; inside each segment one channel ramps as floor(255 i / n)."""
    segments = [(15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False)]
    wheel, row = np.zeros([55, 3]), 0
    for n, full, ramp, rising in segments:
        r = np.floor(255 * np.arange(0, n) / n)
        wheel[row:row + n, full] = 255
        wheel[row:row + n, ramp] = r if rising else 255 - r
        row += n
    return wheel


def flow_to_image(flow):
    """Middlebury colour image (h, w, 3) uint8 of a flow field, numpy on the host, with the reference's dtypes (flow.py:140-220):
    unknown (|.| > 1e7) and NaN components count as 0, the field is scaled by its largest magnitude, hue from the angle, saturation
    from the magnitude.  As in the reference, unknown components of `flow` are zeroed in place."""
    u, v = flow[:, :, 0], flow[:, :, 1]
    unknown = (abs(u) > 1e7) | (abs(v) > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    maxrad = max(-1, np.max(np.sqrt(u ** 2 + v ** 2)))
    u = u / (maxrad + np.finfo(float).eps)
    v = v / (maxrad + np.finfo(float).eps)

    h, w = u.shape
    img = np.zeros([h, w, 3])
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    wheel = _color_wheel()
    ncols = wheel.shape[0]
    rad = np.sqrt(u ** 2 + v ** 2)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    inside = rad <= 1
    for c in range(3):
        col = (1 - f) * (wheel[k0 - 1, c] / 255) + f * (wheel[k1 - 1, c] / 255)
        col[inside] = 1 - rad[inside] * (1 - col[inside])
        col[~inside] *= 0.75
        img[:, :, c] = np.uint8(np.floor(255 * col * (1 - nan)))
    img[np.repeat(unknown[:, :, None], 3, axis=2)] = 0
    return np.uint8(img)


def get_flow_model(args):
    """The flow estimator `--flow_models` names: "tvl1" (alone) -> estimate_tvl1 with the fixed defaults.  The reference's networks
    need downloaded weights that this build does not have; naming one is an error, not a silent substitution."""
    names = flow_model_names(args)
    nets = [m for m in names if m != "tvl1"]
    if "tvl1" not in names or nets:
        raise ValueError(f"--flow_models {','.join(names)}: {', '.join(nets) or 'these models'} need downloaded network weights, "
                         "which this build does not use; pass --flow_models tvl1 for the built-in TV-L1 estimator")
    return lambda im1, im2: estimate_tvl1(im1, im2)


def flow_dir(args):
    return args.output_dir + "/" + name(args.content) + "_" + "_".join([name(s) for s in args.style]) + "/flow/"


def _mask_image(flow_a, flow_b, no_check_occlusion):
    if no_check_occlusion:
        return Image.fromarray(flow_to_image(flow_a)).convert("L")
    return Image.fromarray(check_consistency(flow_a, flow_b)).convert("L")


def write_flow_cache(model, args):
    """The reference's process_content_video loop (load.py:141-188) over a directory of frames: for every pair (a, b) of neighbours,
    the last frame paired with the first, forward_<a>_<b>.flo = model(a, b), backward_<b>_<a>.flo = model(b, a), and the two
    reliability PNGs of the same names.  A pair whose backward PNG (written last) exists is skipped.  Returns the frame paths."""
    fdir = flow_dir(args)
    os.makedirs(fdir, exist_ok=True)
    frames = load.process_content_frames(args.content)
    for a, b in zip(frames, frames[1:] + frames[:1]):
        if os.path.isfile("%s/backward_%s_%s.png" % (fdir, name(b), name(a))):
            continue
        img1 = np.array(Image.open(a).convert("RGB"))
        img2 = np.array(Image.open(b).convert("RGB"))
        forward = model(img1, img2)
        load.write_flow(forward, "%s/forward_%s_%s.flo" % (fdir, name(a), name(b)))
        backward = model(img2, img1)
        load.write_flow(backward, "%s/backward_%s_%s.flo" % (fdir, name(b), name(a)))
        _mask_image(forward, backward, args.no_check_occlusion).save("%s/forward_%s_%s.png" % (fdir, name(a), name(b)))
        _mask_image(backward, forward, args.no_check_occlusion).save("%s/backward_%s_%s.png" % (fdir, name(b), name(a)))
        print("processed optical flow: %s <---> %s" % (name(a), name(b)))
    return frames
