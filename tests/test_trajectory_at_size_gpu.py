"""Optimiser trajectories at the benchmark's sizes, shadowed iterate by iterate by the fp64 oracle (oracle/style_oracle.py).

Whole L-BFGS runs cannot be compared with the oracle: the first steps are chaotic (test_fullsize_gpu.py::test_full_size_lbfgs_descends - a
1e-6 change of the start image moves the third evaluation's loss over two orders of magnitude, in the reference's own arithmetic too).  So
the oracle follows the engine instead of running beside it.  The engine runs PixelOptimizer.step() the way bench.py does (hip_graph on,
default flags); after every step the buffers the replayed graph left are read - the loss slots, the gradient at x_k (engine.gbuf[0]),
the activations and decision bytes, x_{k+1} - and at every iterate:
- evaluation: every loss slot 1e-4 of the fp64 oracle at x_k pinned to the engine's decisions (tests/engine_decisions.py), the gradient
  1e-4 rel-L2 of the pinned fp64 gradient - and, at the first and last iterate, as close to it as the fp32 oracle pinned alike (1.5x);
- update: the oracle's restatement of torch.optim.LBFGS / Adam (reference optim.py:180-196) runs in fp64 on the engine's own sequence of
  losses and gradients, and the engine's move x_{k+1} - x_k is 2e-4 rel-L2 of the oracle's (the bar of
  test_random_shapes_gpu.py::test_random_lbfgs_problems_against_the_oracle) beyond the half fp32 spacing of storing x_{k+1}; L-BFGS ends
  with the same iteration count and history length.
Each check compares the same inputs, so an iterate where the loss spikes is checked like any other."""
import os
import time

import pytest
import torch

import synth
from conftest import NIN_FLAGS, product_args, rel_l2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model,S,optimizer,N", [("vgg19", 1024, "lbfgs", 5), ("vgg19", 512, "lbfgs", 10), ("vgg19", 1024, "adam", 10),
                                                 ("nin", 1024, "lbfgs", 5)])
def test_shadowed_trajectory_at_size(weight_files, model, S, optimizer, N):
    """VGG-19 at 1024 and 512 (bench.py's workload and the size where conv_x3w splits its channel loop), L-BFGS with history 100 and Adam;
    NIN + --use_covariance at 1024 (BASELINE config 5)."""
    import models
    import optim
    from engine_decisions import engine_decisions
    from oracle import OracleNet, adam_run, build_spec, lbfgs_run
    from oracle.style_oracle import loss_order
    t0 = time.time()
    extra = NIN_FLAGS + ["--use_covariance"] if model == "nin" else []
    args = product_args(weight_files, extra, model=model, optimizer=optimizer, S=S, N=N)
    args.hip_graph = True
    content, style, init = synth.images(S)
    optim.set_model_args(args, S)
    net, losses = models.load_model(args)
    optim.set_content_targets(net, content, args)
    optim.set_style_targets(net, [style], args)
    for m in losses:
        m.mode = "loss"
    opt = optim.PixelOptimizer(net, losses, init, args)
    eng = opt.engine
    assert eng is not None and opt.use_graph

    # the launches under test (one eager evaluation at x_0 with the route log on)
    routes = eng.describe_routes(opt.x)
    kernels = {r["kernel"] for r in routes}
    if model == "vgg19":
        # (1024: conv_x3p takes the 64- to 256-channel layers; 512: those run on conv_x3, and conv_x3w splits channel loops)
        assert {"conv_x3q", "conv_x3w", "conv_x3p" if S == 1024 else "conv_x3"} <= kernels, kernels
        assert any(r["kernel"] == "conv_x3w" and r.get("gram") for r in routes), routes
        assert any(r.get("unpool") for r in routes), routes
        if S == 512:
            assert any(r["ksplit"] > 1 for r in routes), routes
    else:   # (NIN: the strided stem runs as a 3x3 conv_x3w over space-to-depth sites; its pools are 3x3 / 2, so nothing unpools)
        assert "conv_x3w" in kernels, kernels

    sd = synth.nin_state_dict() if model == "nin" else synth.vgg19_state_dict()
    nets = {}
    for dt in (torch.float64, torch.float32):
        onet = OracleNet(build_spec(args), sd, dtype=dt)
        onet.capture_content(content)
        onet.capture_style([style], [1.0])
        nets[dt] = onet
    o64 = nets[torch.float64]
    spec = o64.spec
    order = loss_order(spec)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xs, totals, grads, report = [], [], [], []
    try:
        for k in range(N):
            x_k = opt.x.detach().cpu().clone()
            opt.step()
            torch.cuda.synchronize()
            slots, total, g_k = eng.slots.cpu().tolist(), float(eng.total.sum()), eng.gbuf[0].cpu().clone()
            acts, aux = o64._forward(x_k.double())
            decisions, flips = engine_decisions(eng, spec, acts, aux)
            del acts, aux
            _, plosses, pg = o64.feval(x_k, decisions=decisions)
            assert len(slots) == len(order)
            for j, i in enumerate(order):
                want = float(plosses.get(i, 0.0))
                assert abs(slots[j] - want) <= 1e-4 * max(abs(want), 1e-9), (k, spec[i].name, slots[j], want)
            ours = rel_l2(g_k, pg)
            line = f"iterate {k}: loss {total:.6e}, gradient {ours:.2e} from the pinned fp64 oracle, {sum(flips.values())} decisions off fp64"
            assert ours <= 1e-4, (k, ours)
            if k in (0, N - 1):
                theirs = rel_l2(nets[torch.float32].feval(x_k, decisions=decisions)[2], pg)
                line += f" (fp32 oracle pinned alike: {theirs:.2e})"
                assert ours <= 1.5 * theirs, (k, ours, theirs)
            report.append(line)
            xs.append(x_k)
            totals.append(total)
            grads.append(g_k.double().flatten())
        x_end = opt.x.detach().cpu().clone()
    finally:
        torch.set_num_threads(threads)

    # the update: the oracle's optimiser in fp64, fed the engine's own losses and gradients
    seen = []

    def fg(x):
        k = len(seen)
        seen.append(x.clone())
        return totals[k], grads[k]
    x0 = xs[0].double()
    if optimizer == "lbfgs":
        stats = {}
        out, calls = lbfgs_run(fg, x0, N, history=args.lbfgs_num_correction, tol_grad=float(args.lbfgs_tolerance_grad),
                               tol_change=float(args.lbfgs_tolerance_change), stats=stats)
    else:
        out, calls = adam_run(fg, x0, N - 1, lr=args.learning_rate)   # (N - 1 iterations of the reference's driver are N steps)
    assert calls == N
    ends = xs[1:] + [x_end]
    oracle_ends = [t.reshape(x0.shape) for t in seen[1:]] + [out]
    errs = []
    for k in range(N):
        # (the image is fp32: L-BFGS's first move at this size, t = 1 / |g|_1, is mostly below its resolution, so x_{k+1} - x_k is the move
        #  rounded to the image's grid.  Every element of x_{k+1} may sit half an fp32 spacing off x_k + move; what is beyond that is the
        #  error of the move itself, relative to the move)
        move = oracle_ends[k] - seen[k].reshape(x0.shape)
        got = ends[k]
        half_ulp = 0.5 * (torch.nextafter(got.abs(), torch.tensor(float("inf"))) - got.abs()).double()
        beyond = ((got.double() - (xs[k].double() + move)).abs() - half_ulp).clamp_min(0)
        errs.append(float(beyond.norm() / move.norm()))
        report[k] += f"; move {errs[-1]:.2e} from the oracle's beyond rounding (|move| {float(move.norm()):.2e})"
    print(f"{model} {S} {optimizer} N = {N} ({time.time() - t0:.0f} s):\n  " + "\n  ".join(report))
    for k, err in enumerate(errs):
        assert err <= 2e-4, (k, err)
    if optimizer == "lbfgs":
        s = opt.state.status()
        assert s["n_iter"] == stats["n_iter"] == N and s["history_len"] == stats["history_len"], (s, stats)
