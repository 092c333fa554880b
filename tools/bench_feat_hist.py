"""Cost of the feature-histogram kernels (csrc/feat_hist.hip) on one MI355X, beside the plain Gram kernels on the same tensors and beside the
time their algorithmic bytes take at the achievable memory rate, and of a hist_loss_factor job beside the same job without the term.

Kernels: the five VGG-19 style-layer shapes of a 1024 x 1024 image (C x H_l x W_l), 256 bins, 1024 knots (the defaults).  Per shape
  hist fwd   hip.feat_hist_fwd: five launches that read F three times (range, counts, residual); algorithmic bytes 3 x 4 C N + 4 C K;
  hist bwd   hip.feat_hist_bwd: one launch, F read once and gx written once; algorithmic bytes 2 x 4 C N + 4 C K;
  gram fwd / gram bwd   hip.gram_fwd / hip.gram_bwd of the same layer (the kernels every job runs: the baseline, never the new code).
`at rate` is bytes / 6.3 TB/s, the rate a float4 copy reaches on this part; `x rate` = measured median over that time.  The layers below
relu1_1 fit the 256 MiB Infinity Cache with room to spare, so repeated calls read them from there and can come in under 1.
The variants run interleaved, `--rounds` rounds of `--reps` back-to-back calls between device events after a warm-up round; the table gives
the median and the minimum over the rounds.  Feature maps are relu(randn + 0.3), the tables the quantiles of relu(2 randn + 1).

Job: VGG-19 (seeded synthetic weights), 1024 x 1024, default layers, L-BFGS: iterations per second of `--steps` steps after `--warmup` (host
clock around a device synchronise) with hist_loss_factor 0 on the fused engine (the project's normal route), hist_loss_factor 0 on the
module path (autograd over the HIP kernels) and hist_loss_factor 1 (module path, its only route) - all in the same run.

    python tools/bench_feat_hist.py [--rounds 7] [--reps 10] [--steps 20] [--warmup 3] [--size 1024] > profiles/bench_feat_hist.md
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "maua-style_amd")]

RATE = 6.3e12  # bytes / s: float4 copy on an MI355X
BINS, KNOTS = 256, 1024


def layer_shapes(size):
    return [("relu1_1", 64, size, size), ("relu2_1", 128, size // 2, size // 2), ("relu3_1", 256, size // 4, size // 4),
            ("relu4_1", 512, size // 8, size // 8), ("relu5_1", 512, size // 16, size // 16)]


def kernel_table(a, out):
    import hip
    out.append("| layer | C x H x W | hist fwd us (median / min) | at rate us | x rate | hist bwd us (median / min) | at rate us | x rate | "
               "gram fwd us | gram bwd us | hist fwd x gram fwd | hist bwd x gram bwd |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name, C, H, W in layer_shapes(a.size):
        N = H * W
        gen = torch.Generator().manual_seed(C + H)
        f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3).cuda()
        table = hip.feat_hist_quantiles(torch.relu(2 * torch.randn(C, 64, 64, generator=gen) + 1).cuda(), KNOTS)
        d1 = torch.randn(C, C, generator=gen).cuda()
        dsym = (d1 + d1.t()).contiguous()
        gx = torch.empty(C, H, W, device="cuda")
        ws_g = torch.empty(hip.gram_workspace_bytes(C, N), dtype=torch.uint8, device="cuda")
        gram = torch.empty(C, C, device="cuda")
        ws_h = torch.empty(hip.feat_hist_workspace_bytes(C, H, W, BINS, KNOTS), dtype=torch.uint8, device="cuda")
        state = torch.empty(hip.feat_hist_state_bytes(C, BINS) // 4, dtype=torch.int32, device="cuda")
        loss = torch.empty(1, device="cuda")
        up = torch.ones(1, device="cuda")
        variants = {
            "hist fwd": lambda: hip.feat_hist_fwd(f, table, BINS, state=state, loss=loss, workspace=ws_h),
            "hist bwd": lambda: hip.feat_hist_bwd(f, table, state, BINS, 2.0 / (C * N), gx, False, upstream=up),
            "gram fwd": lambda: hip.gram_fwd(f, 1.0 / (C * N), False, out=gram, workspace=ws_g),
            "gram bwd": lambda: hip.gram_bwd(dsym, f, None, gx, False, workspace=ws_g),
        }
        times = {k: [] for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rnd in range(a.rounds + 1):  # round 0 warms up
            for k, fn in variants.items():
                fn()
                ev[0].record()
                for _ in range(a.reps):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                if rnd:
                    times[k].append(ev[0].elapsed_time(ev[1]) / a.reps * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        floor = {"hist fwd": (3 * 4 * C * N + 4 * C * KNOTS) / RATE * 1e6, "hist bwd": (2 * 4 * C * N + 4 * C * KNOTS) / RATE * 1e6}
        out.append(f"| {name} | {C} x {H} x {W} | {med['hist fwd']:.1f} / {min(times['hist fwd']):.1f} | {floor['hist fwd']:.1f} | "
                   f"{med['hist fwd'] / floor['hist fwd']:.2f} | {med['hist bwd']:.1f} / {min(times['hist bwd']):.1f} | {floor['hist bwd']:.1f} | "
                   f"{med['hist bwd'] / floor['hist bwd']:.2f} | {med['gram fwd']:.1f} | {med['gram bwd']:.1f} | "
                   f"{med['hist fwd'] / med['gram fwd']:.2f} | {med['hist bwd'] / med['gram bwd']:.2f} |")
        print(json.dumps(dict(layer=name, C=C, H=H, W=W, **{k.replace(" ", "_") + "_us": v for k, v in med.items()},
                              **{k.replace(" ", "_") + "_at_rate_us": v for k, v in floor.items()})), file=sys.stderr, flush=True)


def job_rates(a, out):
    import config
    import models
    import optim
    import synth
    tmp = tempfile.mkdtemp(prefix="bench_feat_hist_")
    wfile = os.path.join(tmp, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(tmp, "scaling.json")
    with open(scaling, "w") as fh:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, fh)
    S = a.size
    content, style, init = synth.images(S)
    rates = {}
    for label, factor in (("hist_loss_factor 0, fused engine", 0.0), ("hist_loss_factor 0, module path", 0.0), ("hist_loss_factor 1 (module path)", 1.0)):
        preset = os.path.join(tmp, "hist.json")
        with open(preset, "w") as fh:
            json.dump({"hist_loss_factor": factor}, fh)
        args = config.get_args(["--content", "c.png", "--style", "s.png", "--model_file", wfile, "--disable_check", "--scaling_args", scaling,
                                "--image_sizes", str(S), "--num_iters", str(a.steps), "--seed", "0", "--no_hist_match", "--load_args", preset])
        optim.set_model_args(args, S)
        net, losses = models.load_model(args)
        optim.set_content_targets(net, content, args)
        optim.set_style_targets(net, [style], args)
        for m in losses:
            m.mode = "loss"
        opt = optim.PixelOptimizer(net, losses, init, args, planned_iters=a.steps + a.warmup)
        if "module path" in label:
            opt.engine = None
        assert (opt.engine is not None) == ("fused" in label), label
        for _ in range(a.warmup):
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            opt.step()
        torch.cuda.synchronize()
        rates[label] = a.steps / (time.perf_counter() - t0)
        print(json.dumps(dict(job=label, size=S, steps=a.steps, iterations_per_s=rates[label])), file=sys.stderr, flush=True)
        del opt, net, losses
        torch.cuda.empty_cache()
    out.append("| job | iterations/s | ms per iteration |")
    out.append("|---|---|---|")
    for k, v in rates.items():
        out.append(f"| {k} | {v:.2f} | {1e3 / v:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_feat_hist: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    out = [f"# Feature-histogram kernels and a hist_loss_factor job at {a.size} x {a.size} (tools/bench_feat_hist.py)", "",
           f"Device: {torch.cuda.get_device_name(0)}.  Kernel times: median / minimum over {a.rounds} interleaved rounds of {a.reps} calls, device "
           f"events; {BINS} bins, {KNOTS} knots.", "`at rate` = the call's algorithmic bytes (forward 3 reads of F, backward one read of F and "
           "one write of gx, plus the table) at 6.3 TB/s; `x rate` = median over that time.", ""]
    kernel_table(a, out)
    out += ["", f"## Whole job, L-BFGS, {a.steps} steps after {a.warmup}", ""]
    job_rates(a, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
