"""Cost of the guided (per-region) Gram kernels on one MI355X, beside the unguided kernels on the same tensors, and of a guided job beside
the same job unguided.

Kernels: the five VGG-19 style-layer shapes of a 1024 x 1024 image (C x H_l W_l).  Per shape, forward and backward of
  base        hip.gram_fwd / hip.gram_bwd (the kernels every unguided job runs: the baseline, never the new code);
  R1 ones     one region of ones (the same mathematics as the baseline, through csrc/gram_guided.hip);
  R2 / R4 hard   top / bottom halves and 2 x 2 quadrants as one-hot guides (a quadrant's rows are half rows of the plane: at W_l = 64 a
              64-pixel stage holds a whole row, so the left / right split cannot be skipped there);
  R2 / R4 soft   uniform random guides (no stage can be skipped).
The variants run interleaved, `--rounds` rounds of `--reps` back-to-back calls between device events after a warm-up round; the table
gives the median and the minimum over the rounds.  Feature maps are relu(randn): the same data for every variant of a shape.

Job: VGG-19 (seeded synthetic weights), 1024 x 1024, default layers, L-BFGS: iterations per second of `--steps` steps after `--warmup`
(host clock around a device synchronise) for the guided job (R = 4 hard quadrants) on the module path (the default), the same job with the
planner field guided_engine = 1 (the fused engine; launched eagerly like the other rows, and once more replaying its captured graph), the
unguided job on the module path (autograd over the HIP kernels) and the unguided job on the fused engine (the project's normal route).
The kernel table's row "R4 hard, fused finish + masked bwd" is the engine's form of the layer: the forward call whose finishing launch also
forms the MSE, the D matrices and the ledger record (its distance to "R4 hard" is what the fused finish costs over the plain one), and the
backward call with the ReLU mask in its epilogue.

    python tools/bench_guided.py [--rounds 7] [--reps 10] [--steps 20] [--warmup 3] [--size 1024] > profiles/bench_guided.md
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


def hard_guides(R, H, W):
    g = torch.zeros(R, H, W)
    if R == 1:
        g[0] = 1
    elif R == 2:
        g[0, :H // 2], g[1, H // 2:] = 1, 1
    else:
        g[0, :H // 2, :W // 2], g[1, :H // 2, W // 2:], g[2, H // 2:, :W // 2], g[3, H // 2:, W // 2:] = 1, 1, 1, 1
    return g


def kernel_table(a, out):
    import hip
    out.append("| layer | C x HW | variant | forward us (median / min) | x base | backward us (median / min) | x base |")
    out.append("|---|---|---|---|---|---|---|")
    summary = {}
    for name, C, H, W in layer_shapes(a.size):
        N = H * W
        gen = torch.Generator().manual_seed(C + H)
        f = torch.relu(torch.randn(C, N, generator=gen)).cuda()
        d1 = torch.randn(C, C, generator=gen)
        d1 = (d1 + d1.t()).cuda().contiguous()
        gf = torch.empty(C, N, device="cuda")
        ws_b = torch.empty(hip.gram_workspace_bytes(C, N), dtype=torch.uint8, device="cuda")
        gram_b = torch.empty(C, C, device="cuda")
        variants = {"base": (lambda: hip.gram_fwd(f, 1.0 / (C * N), False, out=gram_b, workspace=ws_b),
                             lambda: hip.gram_bwd(d1, f, None, gf, False, workspace=ws_b))}
        keep = []
        for label, R, soft in (("R1 ones", 1, False), ("R2 hard", 2, False), ("R4 hard", 4, False), ("R2 soft", 2, True), ("R4 soft", 4, True)):
            g = (torch.rand(R, N, generator=gen) if soft else hard_guides(R, H, W).reshape(R, N)).cuda().contiguous()
            mass = hip.gram_guided_mass(g)
            scale = (1.0 / (C * mass)).float()
            ws = torch.empty(hip.gram_guided_workspace_bytes(R, C, N), dtype=torch.uint8, device="cuda")
            grams = torch.empty(R, C, C, device="cuda")
            d = d1.expand(R, C, C).contiguous()
            keep.append((g, mass, scale, ws, grams, d))
            variants[label] = (lambda g=g, scale=scale, mass=mass, ws=ws, grams=grams: hip.gram_guided_fwd(f, g, scale, False, mass, out=grams, workspace=ws),
                               lambda g=g, scale=scale, d=d: hip.gram_guided_bwd(d, f, g, scale, None, gf, False))
            if label == "R4 hard":  # the engine's form of the layer: finishing launch with the MSE, D and the ledger record; masked backward
                target, dmat = torch.zeros(R, C, C, device="cuda"), torch.empty(R, C, C, device="cuda")
                ls, gs = torch.full((R,), 1.0 / (C * C), device="cuda"), torch.full((R,), 4.0 / (C * C), device="cuda")
                led = hip.loss_ledger(1, 1, f.device)
                keep.append((target, dmat, ls, gs, led))
                variants["R4 hard, fused finish + masked bwd"] = (
                    lambda g=g, scale=scale, mass=mass, ws=ws, grams=grams, target=target, dmat=dmat, ls=ls, gs=gs, led=led:
                    hip.gram_guided_fwd_mse_ledger(f, g, scale, False, mass, grams, None, target, dmat, ls, gs, led[0], 0, workspace=ws),
                    lambda g=g, scale=scale, d=d: hip.gram_guided_bwd_masked(d, f, g, scale, None, gf, False, relu_mask=f))
        times = {k: ([], []) for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rnd in range(a.rounds + 1):  # round 0 warms up
            for k, fns in variants.items():
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
            out.append(f"| {name} | {C} x {N} | {k} | {med[k][0]:.1f} / {min(v[0]):.1f} | {med[k][0] / med['base'][0]:.2f} | "
                       f"{med[k][1]:.1f} / {min(v[1]):.1f} | {med[k][1] / med['base'][1]:.2f} |")
            print(json.dumps(dict(layer=name, C=C, HW=N, variant=k, fwd_us=med[k][0], bwd_us=med[k][1], fwd_min_us=min(v[0]), bwd_min_us=min(v[1]))),
                  file=sys.stderr, flush=True)
        summary[name] = med
        del keep
    return summary


def job_rates(a, out):
    import config
    import models
    import optim
    import synth
    tmp = tempfile.mkdtemp(prefix="bench_guided_")
    wfile = os.path.join(tmp, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(tmp, "scaling.json")
    with open(scaling, "w") as fh:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, fh)
    S = a.size
    content, style, init = synth.images(S)
    guides = (hard_guides(4, S, S), [hard_guides(4, S, S)])
    rates = {}
    import plan
    for label in ("guided, R = 4 hard quadrants (module path)", "guided, R = 4 hard quadrants, guided_engine=1 (fused engine)",
                  "guided, R = 4 hard quadrants, guided_engine=1 (fused engine, captured graph)", "unguided, module path", "unguided, fused engine"):
        plan.OVERRIDES.pop("guided_engine", None)
        if "guided_engine=1" in label:  # (what MAUA_PLAN="guided_engine=1" sets)
            plan.OVERRIDES["guided_engine"] = "1"
        args = config.get_args(["--content", "c.png", "--style", "s.png", "--model_file", wfile, "--disable_check", "--scaling_args", scaling,
                                "--image_sizes", str(S), "--num_iters", str(a.steps), "--seed", "0", "--no_hist_match"])
        if "captured graph" in label:
            args.hip_graph = 1  # (a job of 128 iterations or more takes the graph by itself; the other rows launch eagerly)
        optim.set_model_args(args, S)
        net, losses = models.load_model(args)
        optim.set_content_targets(net, content, args)
        optim.set_style_targets(net, [style], args, style_guides=guides[1] if label.startswith("guided") else None)
        if label.startswith("guided"):
            for m in net.style_losses:
                m.guide = guides[0].cuda()
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
    plan.OVERRIDES.pop("guided_engine", None)
    out.append("| job | iterations/s |")
    out.append("|---|---|")
    for k, v in rates.items():
        out.append(f"| {k} | {v:.2f} |")
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_guided: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    out = [f"# Guided Gram kernels and a guided job at {a.size} x {a.size} (tools/bench_guided.py)", "",
           f"Device: {torch.cuda.get_device_name(0)}.  Kernel times: median / minimum over {a.rounds} interleaved rounds of {a.reps} calls, device events.",
           "`x base` = median over the median of hip.gram_fwd / hip.gram_bwd on the same tensor.", ""]
    med = kernel_table(a, out)
    out += ["", "R = 4 hard masks relative to R = 1 (medians, forward / backward):", ""]
    for name, m in med.items():
        out.append(f"- {name}: {m['R4 hard'][0] / m['R1 ones'][0]:.2f} / {m['R4 hard'][1] / m['R1 ones'][1]:.2f}"
                   f"  (soft: {m['R4 soft'][0] / m['R1 ones'][0]:.2f} / {m['R4 soft'][1] / m['R1 ones'][1]:.2f})")
    out += ["", f"## Whole job, L-BFGS, {a.steps} steps after {a.warmup}", ""]
    job_rates(a, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
