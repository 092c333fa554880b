"""Neural cellular automaton throughput on one MI355X: the fused CA step (csrc/nca.hip) against a torch-eager restatement of the
reference's CA.forward (NCA_train.py:176-182: pad, conv, 1x1, ReLU, 1x1, rand, add, floor, mul, add) on the same GPU, and training
steps/s at the reference's setting (B = 4, 128^2) with a fixed step_n = 64.  Prints one JSON line; appends it to
profiles/nca_bench.jsonl and writes profiles/nca_bench.md.

    python tools/bench_nca.py [--iters N] [--train_iters N] [--vgg_file F] [--no_write] [--out_dir profiles]

FLOPs are counted from the shapes: per pixel 2 (48 * 96 + 96 * 12) for the two matrix products plus the perception and the
update (~ 11.9 kFLOP); peak = 157.3 TFLOP/s fp32.  The rocprofv3 kernel table is a separate run (`--kernel-trace --stats` over this
script with --iters 20 --no_write)."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "maua-style_amd")]

import hip  # noqa: E402
import nca  # noqa: E402

PEAK_FP32 = 157.3e12


def flops_per_pixel(chn, hidden):
    return 2 * (4 * chn * hidden + hidden * chn) + hidden + chn * 4 * 9 * 2 + 3 * chn


def eager_step(x, w1, b1, w2, filt, rate=0.5):
    """The reference's CA.forward as eager torch launches."""
    b, c, h, w = x.shape
    y = F.conv2d(F.pad(x.reshape(b * c, 1, h, w), [1, 1, 1, 1], "circular"), filt).reshape(b, 4 * c, h, w)
    y = F.conv2d(torch.relu(F.conv2d(y, w1, b1)), w2)
    mask = (torch.rand(b, 1, h, w, device=x.device) + rate).floor()
    return x + y * mask


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_steps(n, size, iters, chn=12, hidden=96):
    ca = nca.NCA.init(chn, hidden, seed=0)
    with torch.no_grad():
        ca.params[-chn * hidden:].normal_(0, 0.01)
    x = torch.rand(n, chn, size, size, device="cuda") * 0.1
    y = torch.empty_like(x)
    state = {"s": 0}

    def fused():
        ca.step(x, seed=0, step=state["s"], out=y)
        state["s"] += 1

    w1, b1, w2 = (t.clone() for t in ca.tensors())
    w1, w2 = w1[:, :, None, None].contiguous(), w2[:, :, None, None].contiguous()
    filt = torch.stack([torch.tensor(f, dtype=torch.float32) for f in
                        ([[0, 0, 0], [0, 1, 0], [0, 0, 0]], [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], [[-1, -2, -1], [0, 0, 0], [1, 2, 1]],
                         [[1, 2, 1], [2, -12, 2], [1, 2, 1]])])[:, None].cuda()

    def eager():
        with torch.no_grad():
            eager_step(x, w1, b1, w2, filt)

    t_f, t_e = timed(fused, iters), timed(eager, iters)
    fl = flops_per_pixel(chn, hidden) * n * size * size
    return {"n": n, "size": size, "fused_us": t_f * 1e6, "eager_us": t_e * 1e6, "fused_steps_s": 1 / t_f, "eager_steps_s": 1 / t_e,
            "fused_tflops": fl / t_f / 1e12, "eager_tflops": fl / t_e / 1e12, "fused_pct_peak": 100 * fl / t_f / PEAK_FP32,
            "speedup": t_e / t_f}


def _vgg(path):
    import models
    seq = models.build_sequential(models.channel_list["VGG-16"], "max")
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(v.shape, generator=g) * ((2.0 / (v.shape[1] * 9)) ** 0.5 if k.endswith("weight") else 0.01)
          for k, v in models.VGG(seq).state_dict().items()}
    torch.save(sd, path)


def bench_train(iters, vgg_file, step_n=64):
    tmp = tempfile.mkdtemp(prefix="nca_bench_")
    if vgg_file is None:
        vgg_file = os.path.join(tmp, "vgg16-397923af.pth")
        _vgg(vgg_file)
    style = nca.StyleModel(vgg_file)
    target = nca.target_grams(style, os.path.join(REPO, "tests", "synth_style_256.png"))
    ca = nca.NCA.init(seed=0)
    tr = nca.Trainer(ca, style, target)
    tr.draw = lambda: (tr.rng.choice(len(tr.pool), tr.batch, replace=False), step_n)
    t = timed(tr.train_step, iters, warmup=2)
    return {"train_step_ms": t * 1e3, "train_steps_s": 1 / t, "step_n": step_n, "batch": 4, "size": 128}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--train_iters", type=int, default=10)
    ap.add_argument("--vgg_file", default=None)
    ap.add_argument("--no_write", action="store_true")
    ap.add_argument("--out_dir", default=os.path.join(REPO, "profiles"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [bench_steps(1, 256, a.iters), bench_steps(1, 1024, max(a.iters // 4, 5)), bench_steps(4, 128, a.iters)]
    train = bench_train(a.train_iters, a.vgg_file) if a.train_iters > 0 else None
    res = {"bench": "nca", "gpu": torch.cuda.get_device_name(0), "steps": rows, "train": train}
    line = json.dumps(res)
    print(line)
    if a.no_write:
        return
    prof = a.out_dir
    os.makedirs(prof, exist_ok=True)
    with open(os.path.join(prof, "nca_bench.jsonl"), "a") as f:
        f.write(line + "\n")
    md = ["# Neural cellular automaton: fused HIP step vs. the torch-eager CA step", "",
          f"One {res['gpu']}; `python tools/bench_nca.py` (times include launch overhead; FLOPs from the shapes, peak 157.3 TF fp32).", "",
          "| B | side | fused us | eager us | fused steps/s | eager steps/s | fused TF/s | % of peak | speed-up |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['n']} | {r['size']} | {r['fused_us']:.1f} | {r['eager_us']:.1f} | {r['fused_steps_s']:.0f} | "
                  f"{r['eager_steps_s']:.0f} | {r['fused_tflops']:.2f} | {r['fused_pct_peak']:.1f} | {r['speedup']:.2f}x |")
    if train:
        md += ["", f"Training (B = 4, 128^2, step_n = {train['step_n']}, VGG-16 style loss on the module path): "
                   f"{train['train_step_ms']:.1f} ms per step, {train['train_steps_s']:.2f} steps/s."]
    with open(os.path.join(prof, "nca_bench.md"), "w") as f:
        f.write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
