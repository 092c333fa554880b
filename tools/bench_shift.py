"""Cost of the shifted Gram kernels (csrc/gram_shift.hip) on one MI355X, beside the plain Gram kernels on the same tensors, and of a
--shift_factor job beside the same job without the term.

Kernels: the five VGG-19 style-layer shapes of a 1024 x 1024 image (C x H_l x W_l).  Per shape, forward and backward of
  base     hip.gram_fwd / hip.gram_bwd (the kernels every job runs: the baseline, never the new code);
  shifts   hip.gram_shift_fwd / hip.gram_shift_bwd with the layer's own shift list (loss.shift_deltas: every delta along x and y), in one call;
  x4 / y4  one shift alone, delta 4 along x and along y (the cost of a single shifted product);
  shifts + mse    what the module path launches for the layer's list: hip.gram_shift_fwd and one hip.mse_fwd_bwd per matrix / hip.gram_shift_bwd;
  shifts fused    what the fused engine launches (StyleLoss.terms_engine): hip.gram_shift_fwd_mse_ledger - matrices, D and the loss record from
                  the finishing launch - / hip.gram_shift_bwd_masked with the ReLU mask in its epilogue.
The variants run interleaved, `--rounds` rounds of `--reps` back-to-back calls between device events after a warm-up round; the table gives
the median and the minimum over the rounds.  Feature maps are relu(randn): the same data for every variant of a shape.

Job: VGG-19 (seeded synthetic weights), 1024 x 1024, default layers, L-BFGS: iterations per second of `--steps` steps after `--warmup` (host
clock around a device synchronise) with --shift_factor 0 on the fused engine (the project's normal route), --shift_factor 0 on the module
path (autograd over the HIP kernels), --shift_factor 1 on the module path (the default route of the shift terms) and --shift_factor 1 with the
preset key terms_engine = 1 (the fused engine and its captured graph) - all in the same run.

    python tools/bench_shift.py [--rounds 7] [--reps 10] [--steps 20] [--warmup 3] [--size 1024] > profiles/bench_shift.md
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


def layer_shapes(size):
    return [("relu1_1", 64, size, size), ("relu2_1", 128, size // 2, size // 2), ("relu3_1", 256, size // 4, size // 4),
            ("relu4_1", 512, size // 8, size // 8), ("relu5_1", 512, size // 16, size // 16)]


def kernel_table(a, out):
    import hip
    import loss
    out.append("| layer | C x H x W | variant | shifts | forward us (median / min) | x base | backward us (median / min) | x base |")
    out.append("|---|---|---|---|---|---|---|---|")
    for name, C, H, W in layer_shapes(a.size):
        N = H * W
        gen = torch.Generator().manual_seed(C + H)
        f = torch.relu(torch.randn(C, H, W, generator=gen)).cuda()
        d1 = torch.randn(C, C, generator=gen).cuda()
        dsym = (d1 + d1.t()).contiguous()
        gf = torch.empty(C, H, W, device="cuda")
        ws_b = torch.empty(hip.gram_workspace_bytes(C, N), dtype=torch.uint8, device="cuda")
        gram_b = torch.empty(C, C, device="cuda")
        variants = {"base": (0, lambda: hip.gram_fwd(f, 1.0 / (C * N), False, out=gram_b, workspace=ws_b),
                             lambda: hip.gram_bwd(dsym, f, None, gf, False, workspace=ws_b))}
        layer = [(axis, d) for d in loss.shift_deltas(H, W) for axis in (0, 1)]
        keep = []
        for label, shifts in (("shifts", layer), ("x4", [(0, 4)]), ("y4", [(1, 4)])):
            if not shifts:
                continue
            S = len(shifts)
            scales = [1.0 / (C * loss.shift_pairs(ax, d, H, W)) for ax, d in shifts]
            ws = torch.empty(hip.gram_shift_workspace_bytes(S, C, H, W), dtype=torch.uint8, device="cuda")
            grams = torch.empty(S, C, C, device="cuda")
            d = d1.expand(S, C, C).contiguous()
            keep.append((ws, grams, d))
            variants[label] = (S, lambda shifts=shifts, scales=scales, ws=ws, grams=grams: hip.gram_shift_fwd(f, shifts, scales, None, out=grams, workspace=ws),
                               lambda shifts=shifts, scales=scales, d=d: hip.gram_shift_bwd(d, f, shifts, scales, None, gf, False))
            if label == "shifts":  # the layer's list finished with the MSE: per matrix (module path) and in the finishing launch (engine)
                target, dm = torch.randn(S, C, C, generator=gen).cuda() / (C * C), torch.empty(S, C, C, device="cuda")
                one, led = torch.zeros(1, device="cuda"), hip.loss_ledger(1, 1, f.device)
                ws_m = torch.empty(hip.reduce_workspace_bytes(C * C), dtype=torch.uint8, device="cuda")
                ls, gs = [1.0 / (C * C)] * S, [2.0 / (C * C)] * S
                keep.append((target, dm, one, led, ws_m))

                def unfused(shifts=shifts, scales=scales, ws=ws, grams=grams, target=target, dm=dm, one=one, ws_m=ws_m, ls=ls, gs=gs):
                    hip.gram_shift_fwd(f, shifts, scales, None, out=grams, workspace=ws)
                    for i in range(len(shifts)):
                        hip.mse_fwd_bwd(grams[i], target[i], dm[i], ls[i], gs[i], False, one, workspace=ws_m)

                variants["shifts + mse"] = (S, unfused, variants[label][2])
                variants["shifts fused"] = (S, lambda shifts=shifts, scales=scales, ws=ws, grams=grams, target=target, dm=dm, led=led, ls=ls, gs=gs:
                                            hip.gram_shift_fwd_mse_ledger(f, shifts, scales, None, grams, target, dm, ls, gs, led[0], 0, workspace=ws),
                                            lambda shifts=shifts, scales=scales, d=d: hip.gram_shift_bwd_masked(d, f, shifts, scales, None, gf, False,
                                                                                                                  relu_mask=f))
        times = {k: ([], []) for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rnd in range(a.rounds + 1):  # round 0 warms up
            for k, (_, *fns) in variants.items():
                for which, fn in enumerate(fns):
                    fn()
                    ev[0].record()
                    for _ in range(a.reps):
                        fn()
                    ev[1].record()
                    torch.cuda.synchronize()
                    if rnd:
                        times[k][which].append(ev[0].elapsed_time(ev[1]) / a.reps * 1e3)
        med = {k: [statistics.median(t) for t in v] for k, v in times.items()}
        for k, v in times.items():
            out.append(f"| {name} | {C} x {H} x {W} | {k} | {variants[k][0] or '-'} | {med[k][0]:.1f} / {min(v[0]):.1f} | {med[k][0] / med['base'][0]:.2f} | "
                       f"{med[k][1]:.1f} / {min(v[1]):.1f} | {med[k][1] / med['base'][1]:.2f} |")
            print(json.dumps(dict(layer=name, C=C, H=H, W=W, variant=k, shifts=variants[k][0], fwd_us=med[k][0], bwd_us=med[k][1],
                                  fwd_min_us=min(v[0]), bwd_min_us=min(v[1]))), file=sys.stderr, flush=True)
        del keep


def job_rates(a, out):
    import config
    import models
    import optim
    import synth
    tmp = tempfile.mkdtemp(prefix="bench_shift_")
    wfile = os.path.join(tmp, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(tmp, "scaling.json")
    with open(scaling, "w") as fh:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, fh)
    S = a.size
    content, style, init = synth.images(S)
    rates = {}
    for label, sf, te in (("--shift_factor 0, fused engine", "0", 0), ("--shift_factor 0, module path", "0", 0), ("--shift_factor 1 (module path)", "1", 0),
                          ("--shift_factor 1, terms_engine 1 (fused engine)", "1", 1)):
        preset = os.path.join(tmp, "terms.json")
        with open(preset, "w") as fh:
            json.dump({"terms_engine": te}, fh)
        args = config.get_args(["--content", "c.png", "--style", "s.png", "--model_file", wfile, "--disable_check", "--scaling_args", scaling,
                                "--image_sizes", str(S), "--num_iters", str(a.steps), "--seed", "0", "--no_hist_match", "--shift_factor", sf,
                                "--load_args", preset])
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
        assert bool(opt.engine is not None and opt.engine.term_steps) == bool(te), label
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
        sys.exit("bench_shift: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    out = [f"# Shifted Gram kernels and a --shift_factor job at {a.size} x {a.size} (tools/bench_shift.py)", "",
           f"Device: {torch.cuda.get_device_name(0)}.  Kernel times: median / minimum over {a.rounds} interleaved rounds of {a.reps} calls, device events.",
           "`x base` = median over the median of hip.gram_fwd / hip.gram_bwd on the same tensor; `shifts` = matrices per call.", ""]
    kernel_table(a, out)
    out += ["", f"## Whole job, L-BFGS, {a.steps} steps after {a.warmup}", ""]
    job_rates(a, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
