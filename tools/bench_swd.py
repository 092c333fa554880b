"""Cost of the sliced Wasserstein kernels (csrc/swd.hip) on one MI355X, beside the plain Gram kernels on the same tensors, beside the unfused
chain of existing entry points that computes the same term, and beside the time the fused design's bytes take at the achievable memory rate;
and of a swd_factor job beside the same job without the term.

Kernels: the five VGG-19 style-layer shapes of a 1024 x 1024 image (C x H_l x W_l), D = C directions, 256 bins, 1024 knots (the defaults).
  swd project   hip.swd_project with a state: P = V F, range slabs, counters zeroed - one launch;
  swd fwd       hip.swd_project + hip.swd_match: the forward of one evaluation, five launches (the match alone cannot be repeated: it leaves G in P);
  swd bwd       hip.swd_bwd: gx = coef upstream V^T G - one launch;
  chain         what the same term costs without csrc/swd.hip: hip.conv1x1_x3 (P = V F, fp16x3 arithmetic) + hip.feat_hist_fwd on P +
                hip.feat_hist_bwd into a second D x N buffer + hip.conv1x1_x3 with V^T - each timed on its own, forward pair and backward
                pair summed;
  gram fwd / gram bwd   hip.gram_fwd / hip.gram_bwd of the same layer (the kernels every job runs).
`at rate` is 28 C N bytes (F in and P out; P for the counts; P in and G out; G in and gF out) at 6.3 TB/s, the rate a float4 copy reaches on
this part; `flops` is 2 x 2 D C N over the forward-plus-backward time of the two products.
The variants run interleaved, `--rounds` rounds of `--reps` back-to-back calls between device events after a warm-up round; the table gives
the medians.  Feature maps are relu(randn + 0.3), the tables the quantiles of the projected relu(2 randn + 1).

Job: VGG-19 (seeded synthetic weights), 1024 x 1024, default layers, L-BFGS: iterations per second of `--steps` steps after `--warmup` (host
clock around a device synchronise) with swd_factor 0 and with swd_factor 1, both on the module path - in the same run.

    python tools/bench_swd.py [--rounds 7] [--reps 10] [--steps 20] [--warmup 3] [--size 1024] > profiles/bench_swd.md
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
    import loss
    out.append("| layer | C x H x W | swd project us | swd fwd us | swd bwd us | fwd + bwd us | at rate us | x rate | products TFLOP/s | "
               "chain fwd us (conv + hist) | chain bwd us (hist + conv) | swd / chain | gram fwd us | gram bwd us |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for index, (name, C, H, W) in enumerate(layer_shapes(a.size)):
        N, D = H * W, C
        gen = torch.Generator().manual_seed(C + H)
        f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3).cuda()
        v = loss.swd_directions(C, D, 0, index).cuda()
        vt = v.t().contiguous()
        smap = torch.relu(2 * torch.randn(C, 64, 64, generator=gen) + 1).cuda()
        table = hip.feat_hist_quantiles(hip.swd_project(smap, v)[0], KNOTS)
        d1 = torch.randn(C, C, generator=gen).cuda()
        dsym = (d1 + d1.t()).contiguous()
        gx = torch.empty(C, H, W, device="cuda")
        proj = torch.empty(D, H, W, device="cuda")
        resid = torch.empty(D, H, W, device="cuda")  # the chain's second D x N buffer
        ws_g = torch.empty(hip.gram_workspace_bytes(C, N), dtype=torch.uint8, device="cuda")
        gram = torch.empty(C, C, device="cuda")
        ws_s = torch.empty(hip.swd_workspace_bytes(C, D, H, W, BINS, KNOTS), dtype=torch.uint8, device="cuda")
        ws_h = torch.empty(hip.feat_hist_workspace_bytes(D, H, W, BINS, KNOTS), dtype=torch.uint8, device="cuda")
        ws_c = torch.empty(max(256, hip.conv1x1_x3_workspace_bytes(1, C, N, D)), dtype=torch.uint8, device="cuda")
        state = torch.empty(hip.swd_state_bytes(D, BINS) // 4, dtype=torch.int32, device="cuda")
        lossv = torch.empty(1, device="cuda")
        up = torch.ones(1, device="cuda")
        f4, p4 = f.unsqueeze(0), proj.unsqueeze(0)

        def swd_fwd():
            hip.swd_project(f, v, BINS, proj=proj, state=state, workspace=ws_s)
            hip.swd_match(proj, table, state, BINS, ws_s, loss=lossv)

        variants = {
            "swd project": lambda: hip.swd_project(f, v, BINS, proj=proj, state=state, workspace=ws_s),
            "swd fwd": swd_fwd,
            "swd bwd": lambda: hip.swd_bwd(proj, vt, 2.0 / (D * N), gx, False, upstream=up),
            "conv fwd": lambda: hip.conv1x1_x3(f4, v, out=p4, workspace=ws_c),
            "hist fwd": lambda: hip.feat_hist_fwd(proj, table, BINS, state=state, loss=lossv, workspace=ws_h),
            "hist bwd": lambda: hip.feat_hist_bwd(proj, table, state, BINS, 2.0 / (D * N), resid, False, upstream=up),
            "conv bwd": lambda: hip.conv1x1_x3(resid.unsqueeze(0), vt, out=gx.unsqueeze(0), workspace=ws_c),
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
        med = {k: statistics.median(t) for k, t in times.items()}
        both = med["swd fwd"] + med["swd bwd"]
        floor = 28.0 * C * N / RATE * 1e6
        tflops = 2 * 2.0 * D * C * N / ((med["swd project"] + med["swd bwd"]) * 1e-6) / 1e12
        chain_f, chain_b = med["conv fwd"] + med["hist fwd"], med["hist bwd"] + med["conv bwd"]
        out.append(f"| {name} | {C} x {H} x {W} | {med['swd project']:.1f} | {med['swd fwd']:.1f} | {med['swd bwd']:.1f} | {both:.1f} | {floor:.1f} | "
                   f"{both / floor:.2f} | {tflops:.1f} | {chain_f:.1f} ({med['conv fwd']:.1f} + {med['hist fwd']:.1f}) | "
                   f"{chain_b:.1f} ({med['hist bwd']:.1f} + {med['conv bwd']:.1f}) | {both / (chain_f + chain_b):.2f} | {med['gram fwd']:.1f} | "
                   f"{med['gram bwd']:.1f} |")
        print(json.dumps(dict(layer=name, C=C, H=H, W=W, **{k.replace(" ", "_") + "_us": t for k, t in med.items()}, at_rate_us=floor)),
              file=sys.stderr, flush=True)
        del f, v, vt, proj, resid, gx, f4, p4
        torch.cuda.empty_cache()


def job_rates(a, out):
    import config
    import models
    import optim
    import synth
    tmp = tempfile.mkdtemp(prefix="bench_swd_")
    wfile = os.path.join(tmp, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(tmp, "scaling.json")
    with open(scaling, "w") as fh:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, fh)
    S = a.size
    content, style, init = synth.images(S)
    rates = {}
    for label, factor in (("swd_factor 0, module path", 0.0), ("swd_factor 1 (module path)", 1.0)):
        preset = os.path.join(tmp, "swd.json")
        with open(preset, "w") as fh:
            json.dump({"swd_factor": factor}, fh)
        args = config.get_args(["--content", "c.png", "--style", "s.png", "--model_file", wfile, "--disable_check", "--scaling_args", scaling,
                                "--image_sizes", str(S), "--num_iters", str(a.steps), "--seed", "0", "--no_hist_match", "--load_args", preset])
        optim.set_model_args(args, S)
        net, losses = models.load_model(args)
        optim.set_content_targets(net, content, args)
        optim.set_style_targets(net, [style], args)
        for m in losses:
            m.mode = "loss"
        opt = optim.PixelOptimizer(net, losses, init, args, planned_iters=a.steps + a.warmup)
        opt.engine = None
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
    for k, r in rates.items():
        out.append(f"| {k} | {r:.2f} | {1e3 / r:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_swd: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    out = [f"# Sliced Wasserstein kernels and a swd_factor job at {a.size} x {a.size} (tools/bench_swd.py)", "",
           f"Device: {torch.cuda.get_device_name(0)}.  Kernel times: medians over {a.rounds} interleaved rounds of {a.reps} calls, device events; "
           f"D = C directions, {BINS} bins, {KNOTS} knots.", "`at rate` = 28 C N bytes at 6.3 TB/s; `x rate` = (swd fwd + swd bwd) over that time; "
           "`products TFLOP/s` = 4 D C N over (swd project + swd bwd); `chain` = the same term from hip.conv1x1_x3, hip.feat_hist_fwd, "
           "hip.feat_hist_bwd and hip.conv1x1_x3, each timed alone in the same run; `swd / chain` = forward plus backward of the one over the other.", ""]
    kernel_table(a, out)
    out += ["", f"## Whole job, L-BFGS, {a.steps} steps after {a.warmup}", ""]
    job_rates(a, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
