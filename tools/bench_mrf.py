"""Cost of the MRF patch-matching kernels (csrc/mrf.hip) on one MI355X, beside the plain Gram kernels on the same tensors and beside the
time their multiply-adds take at the fp32 matrix-core rate, and of an mrf_factor job beside the same job without the term.

Kernels: relu3_1 and relu4_1 (the term's default layers) of 256 x 256, 512 x 512 and 1024 x 1024 VGG-19 jobs, the style image as large as the
job, the bank on the default grid (stride 2, at most 16384 patches).  Per shape
  mrf fwd    hip.mrf_fwd: match (the implicit GEMM, 2 x Q x P x 9 C floating-point operations), merge of the slices' winners, and the loss's
             gather pass; `at rate` is the match's operations at 155 TFLOP/s, what v_mfma_f32_32x32x2f32 sustains on this part, and `of rate`
             that time over the measured median - a lower bound of the match's own share, since the call also merges and gathers;
  mrf bwd    hip.mrf_bwd: one launch, the gather pass again with gx written (the loss pass of the forward call costs about as much);
  mrf bank   hip.mrf_bank: once per capture;
  gram fwd / gram bwd   hip.gram_fwd / hip.gram_bwd of the same layer (the kernels every job runs: the baseline, never the new code).
The variants run interleaved, `--rounds` rounds of `--reps` back-to-back calls between device events after a warm-up round; the table gives
the median and the minimum over the rounds.  Feature maps are relu(randn + 0.3).

Jobs: VGG-19 (seeded synthetic weights) at the three sizes, default style layers, L-BFGS: iterations per second of `--steps` steps after
`--warmup` (host clock around a device synchronise) with mrf_factor 0 on the fused engine (the project's normal route), mrf_factor 0 on
the module path (autograd over the HIP kernels) and mrf_factor 1 on relu3_1 and relu4_1 (module path, its only route) - in the same run.

    python tools/bench_mrf.py [--rounds 5] [--reps 5] [--steps 20] [--warmup 3] [--sizes 256,512,1024] > profiles/bench_mrf.md
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

RATE = 155e12  # floating-point operations / s: v_mfma_f32_32x32x2f32 on an MI355X
STRIDE, MAX_PATCHES = 2, 16384


def layer_shapes(size):
    return [("relu3_1", 256, size // 4, size // 4), ("relu4_1", 512, size // 8, size // 8)]


def kernel_table(a, out):
    import hip
    import loss as loss_mod
    out.append("| job | layer | C x H x W | Q | P | mrf fwd us (median / min) | match at rate us | of rate | TFLOP/s | mrf bwd us (median / min) | "
               "mrf bank us | gram fwd us | gram bwd us | mrf fwd x gram fwd | mrf bwd x gram bwd |")
    out.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for size in a.sizes:
        for name, C, H, W in layer_shapes(size):
            N, Q = H * W, (H - 2) * (W - 2)
            gen = torch.Generator().manual_seed(C + H)
            f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3).cuda()
            s = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3).cuda()
            _, origins = loss_mod.mrf_grid([(H, W)], STRIDE, MAX_PATCHES)
            origin_host = torch.tensor(origins, dtype=torch.int32)
            origin, inv = hip.mrf_bank(s, origin_host)
            P = origin.numel()
            d1 = torch.randn(C, C, generator=gen).cuda()
            dsym = (d1 + d1.t()).contiguous()
            gx = torch.empty(C, H, W, device="cuda")
            ws_g = torch.empty(hip.gram_workspace_bytes(C, N), dtype=torch.uint8, device="cuda")
            gram = torch.empty(C, C, device="cuda")
            ws_m = torch.empty(hip.mrf_workspace_bytes(C, H, W, H, W, P), dtype=torch.uint8, device="cuda")
            state = torch.empty(hip.mrf_state_bytes(H, W) // 4, dtype=torch.int32, device="cuda")
            loss = torch.empty(1, device="cuda")
            up = torch.ones(1, device="cuda")
            variants = {
                "mrf fwd": lambda: hip.mrf_fwd(f, s, origin, inv, state=state, loss=loss, workspace=ws_m),
                "mrf bwd": lambda: hip.mrf_bwd(f, s, origin, state, 2.0 / (9 * C * Q), gx, False, upstream=up),
                "mrf bank": lambda: hip.mrf_bank(s, origin_host),
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
            flop = 2.0 * Q * P * 9 * C
            floor = flop / RATE * 1e6
            out.append(f"| {size} x {size} | {name} | {C} x {H} x {W} | {Q} | {P} | {med['mrf fwd']:.1f} / {min(times['mrf fwd']):.1f} | {floor:.1f} | "
                       f"{floor / med['mrf fwd']:.2f} | {flop / med['mrf fwd'] / 1e6:.1f} | {med['mrf bwd']:.1f} / {min(times['mrf bwd']):.1f} | "
                       f"{med['mrf bank']:.1f} | {med['gram fwd']:.1f} | {med['gram bwd']:.1f} | {med['mrf fwd'] / med['gram fwd']:.1f} | "
                       f"{med['mrf bwd'] / med['gram bwd']:.2f} |")
            print(json.dumps(dict(size=size, layer=name, C=C, H=H, W=W, Q=Q, P=P, flop=flop, match_at_rate_us=floor,
                                  **{k.replace(" ", "_") + "_us": v for k, v in med.items()})), file=sys.stderr, flush=True)


def job_rates(a, out):
    import config
    import models
    import optim
    import synth
    tmp = tempfile.mkdtemp(prefix="bench_mrf_")
    wfile = os.path.join(tmp, "vgg19_synth.pth")
    torch.save(synth.vgg19_state_dict(), wfile)
    scaling = os.path.join(tmp, "scaling.json")
    with open(scaling, "w") as fh:
        json.dump({"100000": {"gpu": "0", "multidevice": False}}, fh)
    out.append("| job | route | iterations/s | ms per iteration |")
    out.append("|---|---|---|---|")
    for S in a.sizes:
        content, style, init = synth.images(S)
        for label, factor in (("mrf_factor 0, fused engine", 0.0), ("mrf_factor 0, module path", 0.0), ("mrf_factor 1 (module path)", 1.0)):
            preset = os.path.join(tmp, "mrf.json")
            with open(preset, "w") as fh:
                json.dump({"mrf_factor": factor}, fh)
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
            rate = a.steps / (time.perf_counter() - t0)
            banks = [int(m.mrf_bank[1].numel()) for m in net.style_losses if getattr(m, "mrf_bank", None) is not None]
            print(json.dumps(dict(job=label, size=S, steps=a.steps, iterations_per_s=rate, bank_patches=banks)), file=sys.stderr, flush=True)
            out.append(f"| {S} x {S} | {label}{' - banks of ' + ', '.join(map(str, banks)) + ' patches' if banks else ''} | {rate:.2f} | {1e3 / rate:.2f} |")
            del opt, net, losses
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=lambda v: [int(x) for x in v.split(",")], default=[256, 512, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mrf: no GPU visible (there is no CPU fallback, and a CPU timing would say nothing)")
    out = [f"# MRF patch-matching kernels and mrf_factor jobs (tools/bench_mrf.py)", "",
           f"Device: {torch.cuda.get_device_name(0)}.  Kernel times: median / minimum over {a.rounds} interleaved rounds of {a.reps} calls, device "
           f"events; bank on the default grid (stride {STRIDE}, at most {MAX_PATCHES} patches) of a style map as large as the working one.",
           "`match at rate` = 2 Q P 9 C floating-point operations at 155 TFLOP/s (fp32 MFMA); `of rate` = that time over the median of the whole "
           "forward call (match, merge and the loss's gather pass): a lower bound of the match's share of the rate.", ""]
    kernel_table(a, out)
    out += ["", f"## Whole jobs, L-BFGS, {a.steps} steps after {a.warmup}", ""]
    job_rates(a, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
