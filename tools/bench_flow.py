"""Time the TV-L1 flow estimator (csrc/flow.hip) on one MI355X: device-event time per frame pair at 1024 x 1024 and 1920 x 1080,
split into solve (one direction), mask and file I/O, and the finest level's TV-L1 iteration in both kernel forms - single-step
launches and the temporally blocked kernel at several k - alternated in the same process, with bytes moved per iteration over
kernel time.  One JSON line per measurement; a summary table on stderr.

    python tools/bench_flow.py [--reps 5] [--ks 4,8,12,16] [--sizes 1024x1024,1920x1080] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "maua-style_amd"), os.path.join(REPO, "tests")]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="4,8,12,16")
    ap.add_argument("--sizes", default="1024x1024,1920x1080")
    ap.add_argument("--quick", action="store_true", help="one repetition, for a kernel trace")
    a = ap.parse_args()
    import flow
    import hip
    import load
    from PIL import Image
    from flow_restatement import synth_texture
    reps = 1 if a.quick else a.reps
    ks = [int(k) for k in a.ks.split(",")]
    rows = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    for spec in a.sizes.split(","):
        w, h = (int(v) for v in spec.split("x"))
        img1 = torch.from_numpy(synth_texture(h, w, 1)).cuda()
        img2 = torch.from_numpy(synth_texture(h, w, 1, dx=1.7, dy=-0.9)).cuda()
        lv = hip.flow_levels(h, w)
        ws = torch.empty(hip.flow_tvl1_workspace_bytes(h, w, lv), dtype=torch.uint8, device="cuda")
        out = torch.empty(2, h, w, device="cuda")
        hip.flow_tvl1(img1, img2, lv, 5, 100, 8, out=out, workspace=ws)  # warm-up (LDS opt-in, code objects)
        torch.cuda.synchronize()

        # whole solve, one direction, each form, alternated
        solve = {k: [] for k in [0] + ks}
        for _ in range(reps):
            for k in solve:
                solve[k] += timed(lambda: hip.flow_tvl1(img1, img2, lv, 5, 100, k, out=out, workspace=ws), 1)
        for k, t in solve.items():
            emit(size=spec, what="solve_one_direction", block_k=k, ms_median=statistics.median(t), ms_all=t, levels=lv, warps=5, iters=100)

        # finest-level iteration: 96 iterations per timed call (a multiple of every k measured below 16 but 16 itself: 6 x 16)
        s0 = torch.zeros(6, h, w, device="cuda")
        s0[:2] = out
        f = hip.flow_warp_prep(hip.flow_grey(img1), hip.flow_grey(img2), s0[:2].contiguous())
        bufs = [s0.clone(), torch.empty_like(s0)]
        n_it = 96

        def run(k):
            cur = 0
            done = 0
            while done < n_it:
                step = 1 if k == 0 else min(k, n_it - done)
                hip.flow_tvl1_step(f, bufs[cur], out=bufs[1 - cur], k=0 if k == 0 else step)
                cur, done = 1 - cur, done + step
        it = {k: [] for k in [0] + ks}
        for _ in range(reps):
            for k in it:
                it[k] += timed(lambda: run(k), 1)
        hw = h * w
        for k, t in it.items():
            us = statistics.median(t) * 1e3 / n_it
            per_launch_bytes = (6 + 3 + 6) * 4 * hw  # state in, fields, state out (interior, compulsory)
            bytes_per_iter = per_launch_bytes / (1 if k == 0 else k)
            emit(size=spec, what="finest_iteration", block_k=k, us_per_iter=us, bytes_per_iter=bytes_per_iter,
                 GB_per_s=bytes_per_iter / (us * 1e-6) / 1e9)

        # mask (both directions) and the files of one pair
        back = hip.flow_tvl1(img2, img1, lv, 5, 100, 8, workspace=ws).clone()
        fwd = out.clone()
        t = []
        for _ in range(reps):
            t += timed(lambda: (hip.flow_consistency(fwd, back), hip.flow_consistency(back, fwd)), 1)
        emit(size=spec, what="mask_both_directions", ms_median=statistics.median(t))
        f_np, b_np = fwd.permute(1, 2, 0).cpu().numpy(), back.permute(1, 2, 0).cpu().numpy()
        m = hip.flow_consistency(fwd, back).cpu().numpy()
        with tempfile.TemporaryDirectory() as d:
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                load.write_flow(f_np, os.path.join(d, "forward.flo"))
                load.write_flow(b_np, os.path.join(d, "backward.flo"))
                Image.fromarray(m).convert("L").save(os.path.join(d, "forward.png"))
                Image.fromarray(m).convert("L").save(os.path.join(d, "backward.png"))
                t.append((time.perf_counter() - t0) * 1e3)
        emit(size=spec, what="file_io_pair", ms_median=statistics.median(t))
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            flow.estimate_tvl1(img1.cpu().numpy(), img2.cpu().numpy())
            t.append((time.perf_counter() - t0) * 1e3)
        emit(size=spec, what="estimate_tvl1_host_call", block_k=flow.TVL1_BLOCK_K, ms_median=statistics.median(t))

    for r in rows:
        keys = ("size", "what", "block_k", "ms_median", "us_per_iter", "GB_per_s")
        sys.stderr.write("  ".join(f"{k}={r[k]:.4g}" if isinstance(r.get(k), float) else f"{k}={r.get(k)}" for k in keys if k in r) + "\n")


if __name__ == "__main__":
    main()
