"""Time style.img_vid on one MI355X with the plan field clip_device at 0 (the reference's host loop: scipy's periodic Gaussian, a host clip,
one download per window) and at 1 (the clip stays on the device, csrc/gauss_wrap.hip): per job the time inside optim.optimize against the
time outside it, then the initial filter alone and every pass of it alone with its achieved bytes per second.

Input per size: a seeded content image (synth.images) and a seeded style clip of 8 frames at half the side (synth.frames), written as
PNGs; `--init random`, one scale, 48 frames, default colour matching.  Every run is a whole job into an empty directory.  The modes
alternate; the first run of each mode is a warm-up (code objects, graph capture) and is reported apart.  optim.optimize and
models.load_model are wrapped with a device synchronisation on both sides, so "outside" is everything else the job does: the noise, the
initial filter, rescaling, colour matching, the roll and temporal blend, the 8-bit conversion and PNG encoding - wherever it runs.

Kernel figures: a pass reads the clip once and writes it once, so its bytes are 2 * T * 3 * S * S * 4; its time is the mean of `--kernel-reps`
back-to-back hip.gauss_wrap calls with one filtered axis between two device events after a warm-up call (each call = the weight-table
kernel + the pass).  The rates are stated against the HBM3E rate of the MI355X: 8.0 TB/s by specification, 6.29 TB/s measured for a copy.

    python tools/bench_img_vid.py [--sizes 256,512] [--frames 48] [--iters 4] [--window 6] [--reps 2] > profiles/bench_img_vid.md

One JSON line per run on stderr, the markdown report on stdout.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "maua-style_amd")]

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--iters", type=int, default=4, help="--num_iters of the job: iterations per window")
    ap.add_argument("--window", type=int, default=6, help="--gram_frame_window of the job")
    ap.add_argument("--reps", type=int, default=2, help="runs per mode after the warm-up run")
    ap.add_argument("--kernel-reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_img_vid: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    import config
    import hip
    import load
    import models
    import optim
    import plan
    import style
    import synth

    sizes = [int(s) for s in a.sizes.split(",")]
    root = tempfile.mkdtemp(prefix="bench_img_vid_")
    wfile = os.path.join(root, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(root, "scaling.json")
    with open(scaling, "w") as f:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, f)

    real_opt, real_load = optim.optimize, models.load_model
    clock = {}

    def timed(key, fn):
        def wrapper(*args, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            clock.setdefault(key, []).append(time.perf_counter() - t)
            return out
        return wrapper

    rows, kernels = [], []
    optim.optimize, models.load_model = timed("optimize", real_opt), timed("load_model", real_load)
    try:
        for size in sizes:
            content = os.path.join(root, f"content_{size}.png")
            load.deprocess(synth.images(size, n=1)[0]).save(content)
            clip = os.path.join(root, f"clip_{size}")
            os.makedirs(clip)
            for i, f in enumerate(synth.frames(8, size // 2)):
                load.deprocess(f[None].clone()).save(os.path.join(clip, f"{i:05d}.png"))

            def job_args(outdir):
                return config.get_args(["--transfer_type", "img_vid", "--content", content, "--style", clip, "--image_sizes", str(size),
                                        "--num_iters", str(a.iters), "--gram_frame_window", str(a.window), "--num_frames", str(a.frames),
                                        "--init", "random", "--model_file", wfile, "--disable_check", "--scaling_args", scaling, "--seed", "0",
                                        "--output_dir", outdir])
            for rep in range(a.reps + 1):
                for mode in ("0", "1"):
                    outdir = os.path.join(root, f"out_{size}_{mode}_{rep}")
                    os.makedirs(outdir)
                    plan.OVERRIDES["clip_device"] = mode
                    clock.clear()
                    torch.manual_seed(0)
                    np.random.seed(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with open(os.devnull, "w") as null:
                        stdout, sys.stdout = sys.stdout, null
                        try:
                            style.img_vid(job_args(outdir))
                        finally:
                            sys.stdout = stdout
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                    written = sorted(os.listdir(outdir))
                    assert len(clock["optimize"]) == 1 and all(len(os.listdir(os.path.join(outdir, d))) == a.frames for d in written), written
                    row = dict(size=size, clip_device=int(mode), run=rep, warm_up=rep == 0, frames=a.frames, window=a.window, iters=a.iters,
                               wall_s=wall, load_model_s=sum(clock["load_model"]), optimize_s=sum(clock["optimize"]))
                    row["outside_s"] = wall - row["load_model_s"] - row["optimize_s"]
                    sys.stderr.write(json.dumps(row) + "\n")
                    rows.append(row)
                    shutil.rmtree(outdir)

            # the initial filter alone, and its passes alone
            torch.manual_seed(0)
            noise = torch.randn((a.frames, 3, size, size)) * 255
            t0 = time.perf_counter()
            import scipy.ndimage as ndi
            host = ndi.gaussian_filter(noise.numpy(), [a.frames, 0, size / 32, size / 32], mode="wrap")
            host_s = time.perf_counter() - t0
            x = noise.cuda()
            full = (float(a.frames), size / 32, size / 32)
            ours = hip.gauss_wrap(x, full)
            err = float((ours.cpu() - torch.from_numpy(host)).norm() / torch.from_numpy(host).norm())
            nbytes = 2 * x.numel() * 4
            for name, sig, roll in (("initial filter, all three passes", full, 0), ("T pass alone", (full[0], 0, 0), 0), ("H pass alone", (0, full[1], 0), 0),
                                    ("W pass alone", (0, 0, full[2]), 0), ("between scales: roll 7 + blend 0.5 along T", (0.5, 0, 0), 7)):
                ws = torch.empty(max(1, hip.lib().maua_gauss_wrap_workspace_bytes(*x.shape, *(float(s) for s in sig))), dtype=torch.uint8, device="cuda")
                out = torch.empty_like(x)
                ms = device_ms(lambda: hip.gauss_wrap(x, sig, roll=roll, workspace=ws, out=out), a.kernel_reps)
                passes = sum(s > 1e-15 for s in sig)
                taps = [min(2 * int(4.0 * s + 0.5) + 1, ext) for s, ext in zip(sig, (a.frames, size, size)) if s > 1e-15]
                k = dict(size=size, what=name, sigmas=sig, taps=taps, ms=ms, bytes=passes * nbytes, rate=passes * nbytes / (ms * 1e-3),
                         host_scipy_s=host_s if passes == 3 else None, rel_l2_vs_host=err if passes == 3 else None)
                sys.stderr.write(json.dumps(k) + "\n")
                kernels.append(k)
    finally:
        optim.optimize, models.load_model = real_opt, real_load
        plan.OVERRIDES.pop("clip_device", None)
        shutil.rmtree(root, ignore_errors=True)

    print("# img_vid: host clip against the device-resident clip\n")
    print(f"`python tools/bench_img_vid.py --sizes {a.sizes} --frames {a.frames} --iters {a.iters} --window {a.window} --reps {a.reps}` on one MI355X "
          f"({torch.cuda.get_device_name(0)}).")
    print(f"Job: one seeded content image, a seeded style clip of 8 frames at half the side, `--init random`, {a.frames} frames, one scale, windows of")
    print(f"{a.window} frames, {a.iters} L-BFGS iterations per window, default colour matching; every run a whole job into an empty directory.")
    print("`outside` = wall - load_model - optimize, with the device synchronised around optimize and load_model: the noise, the initial")
    print("filter, rescaling, colour matching, the roll and temporal blend, the 8-bit conversion and the PNG files.\n")
    print("| size | clip_device | run | wall s | load_model s | inside optimize s | outside optimize s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['size']} | {r['clip_device']} | {'warm-up' if r['warm_up'] else r['run']} | {r['wall_s']:.3f} | {r['load_model_s']:.3f} | "
              f"{r['optimize_s']:.3f} | {r['outside_s']:.3f} |")
    print()
    for size in sizes:
        med = {m: {k: statistics.median(r[k] for r in rows if r["size"] == size and r["clip_device"] == m and not r["warm_up"])
                   for k in ("optimize_s", "outside_s", "wall_s")} for m in (0, 1)}
        print(f"Medians of the measured runs at {size}: host clip {med[0]['optimize_s']:.3f} s inside optimize + {med[0]['outside_s']:.3f} s outside, "
              f"device clip {med[1]['optimize_s']:.3f} s inside + {med[1]['outside_s']:.3f} s outside: "
              f"{med[0]['outside_s'] / max(med[1]['outside_s'], 1e-9):.1f}x less time outside optimize, {med[0]['wall_s'] / med[1]['wall_s']:.2f}x the job rate.\n")
    print("## The periodic Gaussian alone (csrc/gauss_wrap.hip)\n")
    print(f"Clip ({a.frames}, 3, S, S), sigmas (T, S/32, S/32) as `--init random` sets them.  Call time = mean of {a.kernel_reps} back-to-back calls between two")
    print("device events after a warm-up call (weight-table kernel + passes, caller's workspace and output).  Bytes = one read and one write of the")
    print(f"clip per pass.  Share of HBM = achieved rate over {HBM_SPEC / 1e12:.1f} TB/s (specification) and over {HBM_COPY / 1e12:.2f} TB/s (measured copy rate).")
    print("scipy = the host path's `gaussian_filter(..., mode=\"wrap\")` on the same array, one thread, once.\n")
    print("| S | what | taps per filtered axis | call ms | GB moved | achieved TB/s | of 8.0 TB/s | of 6.29 TB/s | scipy s | rel-L2 against scipy |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for k in kernels:
        print(f"| {k['size']} | {k['what']} | {k['taps']} | {k['ms']:.3f} | {k['bytes'] / 1e9:.3f} | {k['rate'] / 1e12:.3f} | {100 * k['rate'] / HBM_SPEC:.1f} % | "
              f"{100 * k['rate'] / HBM_COPY:.1f} % | {'' if k['host_scipy_s'] is None else format(k['host_scipy_s'], '.2f')} | "
              f"{'' if k['rel_l2_vs_host'] is None else format(k['rel_l2_vs_host'], '.1e')} |")


if __name__ == "__main__":
    main()
