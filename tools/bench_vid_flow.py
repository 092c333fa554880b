"""Time the flow-guided vid_img loop (style._vid_img_flow) on one MI355X with the plan field temporal_device at 0 (the reference's host
loop around optim.optimize) and at 1 (frames, warp grid, mask and blend on the device, csrc/warp.hip): frames per second, and per frame
the time inside optim.optimize against the time outside it.

Input: a seeded synthetic clip (synth.frames), its TV-L1 flow cache written once (flow.write_flow_cache) and copied for every run; one
size, two passes.  Every run is a whole job into an empty directory.  The modes alternate; the first run of each mode is a warm-up
(code objects, graph capture) and is reported apart.  optim.optimize and models.load_model are wrapped with a device synchronisation
on both sides, so "outside" is everything else the job does: decoding, rescaling, warp grid, warp, mask, blend, colour matching,
8-bit conversion, PNG encoding - wherever it runs.

    python tools/bench_vid_flow.py [--frames 12] [--size 512] [--iters 50] [--reps 2] > profiles/bench_vid_flow.md

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50, help="--num_iters of the job: iterations per frame over both passes")
    ap.add_argument("--reps", type=int, default=2, help="runs per mode after the warm-up run")
    a = ap.parse_args()
    import config
    import flow
    import load
    import models
    import optim
    import plan
    import style
    import synth

    root = tempfile.mkdtemp(prefix="bench_vid_flow_")
    clip = os.path.join(root, "clip")
    os.makedirs(clip)
    for i, f in enumerate(synth.frames(a.frames, a.size)):
        load.deprocess(f[None].clone()).save(os.path.join(clip, f"{i:05d}.png"))
    wfile = os.path.join(root, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(root, "scaling.json")
    with open(scaling, "w") as f:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, f)

    def job_args(outdir, extra=()):
        return config.get_args(["--transfer_type", "vid_img", "--content", clip, "--style", os.path.join(REPO, "tests", "synth_style_256.png"),
                                "--image_sizes", str(a.size), "--num_iters", str(a.iters), "--passes_per_scale", "2", "--init", "prev_warp",
                                "--model_file", wfile, "--disable_check", "--scaling_args", scaling, "--seed", "0", "--output_dir", outdir]
                               + list(extra))

    cache = os.path.join(root, "cache")
    t0 = time.perf_counter()
    with open(os.devnull, "w") as null:  # (the estimator reports every pair on stdout, where the report goes)
        stdout, sys.stdout = sys.stdout, null
        try:
            flow.write_flow_cache(flow.get_flow_model(job_args(cache, ["--flow_models", "tvl1"])), job_args(cache, ["--flow_models", "tvl1"]))
        finally:
            sys.stdout = stdout
    torch.cuda.synchronize()
    flow_s = time.perf_counter() - t0
    job = "clip_synth_style_256"

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

    rows = []
    optim.optimize, models.load_model = timed("optimize", real_opt), timed("load_model", real_load)
    try:
        for rep in range(a.reps + 1):
            for mode in ("0", "1"):
                outdir = os.path.join(root, f"out_{mode}_{rep}")
                shutil.copytree(os.path.join(cache, job, "flow"), os.path.join(outdir, job, "flow"))
                plan.OVERRIDES["temporal_device"] = mode
                clock.clear()
                torch.manual_seed(0)
                np.random.seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with open(os.devnull, "w") as null:
                    stdout, sys.stdout = sys.stdout, null
                    try:
                        style.vid_img(job_args(outdir))
                    finally:
                        sys.stdout = stdout
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                calls = len(clock["optimize"])
                files = len([f for f in os.listdir(os.path.join(outdir, job, str(a.size))) if f.endswith(".png")])
                assert calls == files == 2 * a.frames, (calls, files)
                row = dict(temporal_device=int(mode), run=rep, warm_up=rep == 0, frames=a.frames, size=a.size, iters_per_call=a.iters // 2,
                           calls=calls, wall_s=wall, load_model_s=sum(clock["load_model"]), optimize_s=sum(clock["optimize"]),
                           optimize_ms_per_call=1e3 * statistics.median(clock["optimize"]))
                row["outside_ms_per_call"] = 1e3 * (wall - row["load_model_s"] - row["optimize_s"]) / calls
                row["calls_per_s"] = calls / (wall - row["load_model_s"])
                sys.stderr.write(json.dumps(row) + "\n")
                rows.append(row)
                shutil.rmtree(outdir)
    finally:
        optim.optimize, models.load_model = real_opt, real_load
        plan.OVERRIDES.pop("temporal_device", None)
        shutil.rmtree(root, ignore_errors=True)

    print("# Flow-guided vid_img: host loop against the device-resident loop\n")
    print(f"`python tools/bench_vid_flow.py --frames {a.frames} --size {a.size} --iters {a.iters} --reps {a.reps}` on one MI355X "
          f"({torch.cuda.get_device_name(0)}).")
    print(f"Clip: {a.frames} seeded frames of {a.size} x {a.size}, TV-L1 flow cache written once ({flow_s:.2f} s for {a.frames} pairs, both")
    print(f"directions, masks and files); one size, two passes, {a.iters // 2} L-BFGS iterations per optimize call, default colour matching;")
    print("every run a whole job into an empty directory.  A call is one frame of one pass.  `outside` = (wall - load_model - optimize) /")
    print("calls, with the device synchronised around optimize and load_model.\n")
    print("| temporal_device | run | wall s | load_model s | optimize ms / call (median) | outside ms / call | frames / s (calls / s without load_model) |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['temporal_device']} | {'warm-up' if r['warm_up'] else r['run']} | {r['wall_s']:.3f} | {r['load_model_s']:.3f} | "
              f"{r['optimize_ms_per_call']:.2f} | {r['outside_ms_per_call']:.2f} | {r['calls_per_s']:.2f} |")
    med = {m: {k: statistics.median(r[k] for r in rows if r["temporal_device"] == m and not r["warm_up"])
               for k in ("optimize_ms_per_call", "outside_ms_per_call", "calls_per_s")} for m in (0, 1)}
    print(f"\nMedians of the measured runs: host loop {med[0]['calls_per_s']:.2f} frames/s ({med[0]['optimize_ms_per_call']:.2f} ms inside "
          f"optimize, {med[0]['outside_ms_per_call']:.2f} ms outside), device loop {med[1]['calls_per_s']:.2f} frames/s "
          f"({med[1]['optimize_ms_per_call']:.2f} ms inside, {med[1]['outside_ms_per_call']:.2f} ms outside): "
          f"{med[1]['calls_per_s'] / med[0]['calls_per_s']:.2f}x the frame rate, {med[0]['outside_ms_per_call'] / max(med[1]['outside_ms_per_call'], 1e-9):.1f}x "
          "less time outside optimize.")


if __name__ == "__main__":
    main()
