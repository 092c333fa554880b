"""The shift and mirror terms of the style loss on the fused engine and its captured graph (preset key terms_engine = 1), end to end on the
GPU: against the fp64 restatement (tests/flip_restatement.py: shift + mirrors + covariance), against the same tree's module path, and
against itself (graph / eager, fresh / reused network).

Bars (those of tests/test_flip_style_gpu.py): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4; trajectories
relL2(ours, f64) <= max(1e-3, 2 relL2(restatement in fp32, f64))."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import flip_restatement as fr
import synth
from conftest import PKG, make_cfg, product_args, rel_l2
from test_flip_style_gpu import TOL_GRAD, TOL_LOSS, prepared, preset_args

pytestmark = pytest.mark.gpu

ALL = dict(shift_factor=0.5, flip_factor=0.5, rotation_factor=0.25)


def config(over, flags=(), size=64, **cfg):
    """restatement fields `over` -> (cfg, preset keys, flags): shift_factor is a flag, the mirror factors and the switch are preset keys."""
    preset = {k: v for k, v in over.items() if k in ("flip_factor", "rotation_factor")}
    preset["terms_engine"] = 1
    flags = list(flags) + (["--shift_factor", str(over["shift_factor"])] if "shift_factor" in over else [])
    return dict(cfg=make_cfg(**over, **cfg), preset=preset, flags=flags, size=size)


def vgg40x56():
    gen = torch.Generator().manual_seed(11)
    content = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 150, 130, generator=gen) * 255 - 120  # (relu1_1: shifts [4, 16] here, [4] in s1 and in the working image)
    init = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    p = config(ALL, ["--style_blend_weights", "0.3,0.9"], size=56, style_blend_weights=[0.25, 0.75])
    return dict(p, content=content, styles=[s1, s2], init=init, kw=dict(S=56, styles=("s1.png", "s2.png")))


def square(size, over, flags=(), **cfg):
    content, style, init = synth.images(size)
    return dict(config(over, flags, size, **cfg), content=content, styles=[style], init=init, kw=dict(S=size))


CONFIGS = {
    "vgg19-64-shift": lambda: square(64, dict(shift_factor=0.5)),
    "vgg19-64-flip": lambda: square(64, dict(flip_factor=0.5)),
    "vgg19-64-rotation-covariance": lambda: square(64, dict(rotation_factor=0.5, use_covariance=True), ["--use_covariance"]),
    "vgg19-64-all": lambda: square(64, ALL),
    "vgg19-64-all-no-grad-norm": lambda: square(64, ALL, ["--no_grad_norm"], normalize_gradients=False),
    "vgg19-64-all-vsf-0": lambda: square(64, ALL, ["--video_style_factor", "0"], video_style_factor=0.0),
    "vgg19-128-shift": lambda: square(128, dict(shift_factor=0.5)),  # relu1_1: deltas [4, 16]
    "vgg19-40x56-two-styles-all": vgg40x56,
}


def compare(name, slots, total, grad, slots_r, total_r, grad_r):
    for k, (a, b) in enumerate(zip(slots, slots_r)):
        print(f"  {name} slot {k}: {a:.9e} ({b:.9e})")
        assert abs(a - b) <= TOL_LOSS * abs(b), (name, k, a, b)
    assert abs(total - total_r) <= TOL_LOSS * abs(total_r), (name, total, total_r)
    e = rel_l2(grad, grad_r)
    print(f"  {name}: pixel gradient rel-L2 {e:.3e}")
    assert e <= TOL_GRAD, (name, e)


def check_plan(eng, shape):
    """Every style layer that has a term is a terms step, and no whole-plane fusion carries one."""
    import loss
    eng._prepare(torch.empty(shape, device="cuda"))
    hw = {0: shape[2:]}
    seen = 0
    for s in eng.steps:
        if s.kind in ("conv", "pool"):
            hw[s.dst] = tuple(eng.gbuf[s.dst].shape[2:])
        if s.kind != "style":
            continue
        h, w = hw[s.src]
        has = (s.mod.shift_factor > 0 and bool(loss.shift_deltas(h, w))) or bool(s.mod.mirror_kinds())
        assert (id(s) in eng.term_steps) == has, (s.mod.name, h, w)
        seen += has
    fused = [id(v[0]) for v in eng.fused_gram.values()] + [id(v[0]) for v in eng.image_gram.values()]
    assert not set(fused) & set(eng.term_steps), "a whole-plane fusion was planned for a terms step"
    return seen


@pytest.mark.parametrize("name", list(CONFIGS), ids=list(CONFIGS))
def test_evaluation_against_fp64_and_the_module_path(tmp_path, weight_files, name):
    from oracle.style_oracle import loss_order
    p = CONFIGS[name]()
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    ref = fr.build(p["content"].double(), [s.double() for s in p["styles"]], p["cfg"], sd)
    total_r, losses_r, grad_r = ref.feval(p["init"].double())
    args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], **p["kw"])
    net, losses, opt = prepared(args, p["content"], p["styles"], p["init"], p["size"])
    assert all(m.terms_engine for m in net.style_losses)
    slots, total, grad = opt.feval()
    torch.cuda.synchronize()
    assert opt.engine is not None, "the network left the engine"
    terms = check_plan(opt.engine, tuple(p["init"].shape))
    # (a mirror exists for every map; shift alone: the maps of 32 pixels and more - relu1_1, relu2_1 and, from 128 pixels, relu3_1)
    assert terms == (5 if p["preset"].keys() & {"flip_factor", "rotation_factor"} else 3 if name == "vgg19-128-shift" else 2), terms
    if name == "vgg19-128-shift":
        first = next(s for s in opt.engine.steps if s.kind == "style")
        assert opt.engine.term_steps[id(first)]["shifts"] == [(0, 4), (1, 4), (0, 16), (1, 16)]
    got = (slots.cpu().double().tolist(), float(total), grad.cpu().clone())
    order = loss_order(ref.spec)
    assert len(order) == len(losses) == len(got[0])
    want = [float(losses_r[i]) if i in losses_r else 0.0 for i in order]
    compare("engine vs fp64", got[0], got[1], got[2], want, float(total_r), grad_r)
    slots_m, total_m, grad_m = opt._feval_modules()
    torch.cuda.synchronize()
    compare("engine vs module path", got[0], got[1], got[2], slots_m.cpu().double().tolist(), float(total_m), grad_m.cpu())


_REFS = {}


def trajectory_refs(opt_name):
    if opt_name not in _REFS:
        cfg = make_cfg(optimizer=opt_name, **ALL)
        content, style, init = synth.images(64)
        ref64 = fr.optimize(content.double(), [style.double()], init.double(), 5, cfg, synth.vgg19_state_dict(dtype=torch.float64), torch.float64)
        ref32 = fr.optimize(content, [style], init, 5, cfg, synth.vgg19_state_dict(), torch.float32)
        _REFS[opt_name] = (content, style, init, ref64, ref32)
    return _REFS[opt_name]


def five_iterations(tmp_path, weight_files, opt_name, hip_graph):
    import optim
    content, style, init, ref64, ref32 = trajectory_refs(opt_name)
    p = config(ALL)
    args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], optimizer=opt_name, S=64, N=5)
    args.hip_graph = hip_graph
    out = optim.optimize(content, [style], init.clone(), 5, args)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    floor, err = rel_l2(ref32, ref64), rel_l2(out, ref64)
    print(f"{opt_name} (hip_graph={hip_graph}): relL2(ours, f64) {err:.3e}, relL2(restatement in fp32, f64) {floor:.3e}")
    assert err <= max(1e-3, 2 * floor), (err, floor)
    assert rel_l2(out, init) > 1e-3  # (it moved)
    return out


def test_five_lbfgs_iterations_graph_and_eager(tmp_path, weight_files, monkeypatch):
    import optim
    engines = []
    keep = optim.PixelOptimizer.step

    def step(self):
        engines.append((self.engine is not None and bool(self.engine.term_steps), self._graph is not None))
        return keep(self)

    monkeypatch.setattr(optim.PixelOptimizer, "step", step)
    graph = five_iterations(tmp_path, weight_files, "lbfgs", 1)
    assert all(e for e, _ in engines) and any(g for _, g in engines), "the job did not replay a captured L-BFGS iteration"
    del engines[:]
    eager = five_iterations(tmp_path, weight_files, "lbfgs", 0)
    assert all(e for e, _ in engines) and not any(g for _, g in engines)
    assert torch.equal(graph, eager), "captured graph and eager launches disagree"


def test_five_adam_steps(tmp_path, weight_files):
    five_iterations(tmp_path, weight_files, "adam", 0)


def test_a_changed_factor_drops_the_bundle(tmp_path, weight_files):
    """One network, two calls with captured iterations kept as bundles; between them every factor changes.  The second call equals the same
    call on a fresh network bit for bit: no captured iteration outlives the coefficients it baked in."""
    import models
    import optim
    content, style, init = synth.images(64)
    after = dict(shift_factor=1.0, flip_factor=0.25, rotation_factor=0.5)

    def network(over):
        p = config(over)
        args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], S=64, N=3)
        args.hip_graph, args._maua_repeated_calls = 1, True  # (iterations captured as bundles that the next call on the network may replay)
        optim.set_model_args(args, 64)
        return (args,) + tuple(models.load_model(args))

    def run(n):
        args, net, losses = n
        out = optim.optimize(content, [style], init.clone(), 3, args, net=net, losses=losses)
        assert net._maua_engine.term_steps and net._maua_engine.iter_graphs
        return out

    shared = network(ALL)
    first = run(shared)
    assert torch.equal(run(shared), first), "the same call again (a replayed bundle) differs"
    key = shared[1]._maua_engine._graph_key()
    for m in shared[1].style_losses:
        m.shift_factor, m.flip_factor, m.rotation_factor = after["shift_factor"], after["flip_factor"], after["rotation_factor"]
    shared[0].shift_factor = after["shift_factor"]
    second = run(shared)
    assert shared[1]._maua_engine._graph_key() != key
    assert torch.equal(second, run(network(after))), "changed factors: a stale graph was served"
    assert not torch.equal(second, first)


def test_debug_poison_changes_nothing(tmp_path, weight_files, monkeypatch):
    import plan
    p = CONFIGS["vgg19-64-all"]()
    results = []
    for poison in ("0", "1"):
        monkeypatch.setitem(plan.OVERRIDES, "debug_poison", poison)
        args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], S=64)
        net, losses, opt = prepared(args, p["content"], p["styles"], p["init"], 64)
        slots, total, grad = opt.feval()
        torch.cuda.synchronize()
        assert opt.engine is not None and opt.engine.term_steps
        results.append((slots.cpu().clone(), total.cpu().clone(), grad.cpu().clone(), opt.engine._graph_key()))
    for a, b in zip(results[0][:3], results[1][:3]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


@pytest.mark.parametrize("over,message", [(dict(shift_factor=0.5), "shifted StyleLoss runs on the module path"),
                                          (dict(flip_factor=0.5), "mirrored StyleLoss runs on the module path")], ids=["shift", "flip"])
def test_switch_off_keeps_the_module_path(tmp_path, weight_files, over, message):
    import engine
    import optim
    p = square(64, over)
    p["preset"]["terms_engine"] = 0
    net, losses, opt = prepared(preset_args(tmp_path, weight_files, p["preset"], p["flags"], S=64), p["content"], p["styles"], p["init"], 64)
    assert not any(m.terms_engine for m in net.style_losses)
    opt.feval()
    assert opt.engine is None and optim._engine_of(net) is None and not hasattr(net, "_maua_engine")
    with pytest.raises(engine.UnsupportedNet, match=message):
        engine.StyleEngine(net, losses)


def test_what_the_engine_refuses_runs_on_the_module_path(tmp_path, weight_files):
    """Shift terms in the covariance form, and two frames per evaluation: UnsupportedNet from the engine, and optim.optimize still finishes."""
    import engine
    import optim
    p = square(64, dict(shift_factor=0.5, use_covariance=True), ["--use_covariance"])
    args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], S=64, N=5)
    net, losses, opt = prepared(args, p["content"], p["styles"], p["init"], 64)
    assert opt.engine is None  # (the L-BFGS optimiser prepares the engine when it is built, and was refused)
    eng = engine.StyleEngine(net, losses)
    with pytest.raises(engine.UnsupportedNet, match="use_covariance"):
        eng.feval(p["init"].cuda())
    out = optim.optimize(p["content"], p["styles"], p["init"].clone(), 5, args)
    assert rel_l2(out, p["init"]) > 1e-3 and bool(torch.isfinite(out).all())

    p = square(64, dict(flip_factor=0.5))
    args = preset_args(tmp_path, weight_files, p["preset"], p["flags"], S=64, N=5)
    net, losses, opt = prepared(args, p["content"], p["styles"], p["init"], 64)
    assert opt.engine is not None
    two = torch.cat([p["init"], p["init"].flip(3)]).cuda()
    with pytest.raises(engine.UnsupportedNet, match="one frame per evaluation"):
        opt.engine.feval(two)
    # (optim.optimize takes one frame per call; an optimiser over a window of two evaluates them module by module)
    frames = optim.PixelOptimizer(net, losses, two.cpu(), args)
    assert frames.engine is None
    for _ in range(2):
        frames.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(frames.x).all()) and rel_l2(frames.x.cpu(), two.cpu()) > 0


def test_cli_with_the_preset_keys(tmp_path, weight_files):
    """style.py --load_args sym.json --image_sizes 64 --num_iters 5 finishes, and its picture differs from the run's without the preset."""
    scaling = tmp_path / "scaling.json"
    scaling.write_text(json.dumps({"100000": {"gpu": "0", "multidevice": False}}))
    preset = tmp_path / "sym.json"
    preset.write_text(json.dumps({"flip_factor": 1.0, "terms_engine": 1}))
    rng = np.random.RandomState(4)
    content, style = tmp_path / "content.png", tmp_path / "style.png"
    Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(content)
    Image.fromarray(rng.randint(0, 256, (80, 80, 3), dtype=np.uint8)).save(style)
    images = {}
    for label, extra in (("sym", ["--load_args", str(preset)]), ("plain", [])):
        out = tmp_path / label
        out.mkdir()
        r = subprocess.run([sys.executable, os.path.join(PKG, "style.py"), "--content", str(content), "--style", str(style), *extra,
                            "--image_sizes", "64", "--num_iters", "5", "--model_file", weight_files["vgg19"], "--disable_check", "--scaling_args",
                            str(scaling), "--seed", "0", "--no_hist_match", "--init", "content", "--output_dir", str(out)], cwd=PKG,
                           env=dict(os.environ, PYTHONPATH=PKG), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["content_style_64.png"]
        images[label] = np.asarray(Image.open(out / "content_style_64.png")).astype(np.int32)
    assert images["sym"].shape == (64, 64, 3)
    assert np.abs(images["sym"] - images["plain"]).max() > 0
