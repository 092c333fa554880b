"""Guided style transfer on the fused engine and its captured graph (planner field guided_engine = 1), end to end on the GPU: against the
fp64 restatement (tests/guided_restatement.py), against the same tree's module path, and against itself (graph / eager, fresh / reused
network).

Bars (those of tests/test_guided_style_gpu.py): per-slot losses <= 1e-5 relative, pixel gradient rel-L2 <= 1e-4; trajectories
relL2(ours, f64) <= max(1e-3, 2 relL2(restatement in fp32, f64))."""
import pytest
import torch

import guided_restatement as gr
import synth
from conftest import NIN_FLAGS, NIN_LAYERS, make_cfg, product_args, rel_l2
from test_guided_style_gpu import TOL_GRAD, TOL_LOSS, halves, prepared

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guided_engine_on(monkeypatch):
    import plan
    monkeypatch.setitem(plan.OVERRIDES, "guided_engine", "1")


def vgg64(extra=(), **cfg):
    content, style, init = synth.images(64)
    guides = (halves(2, 64, 64), [halves(2, 64, 64, vertical=False)])
    return dict(cfg=make_cfg(**cfg), flags=list(extra), kw=dict(S=64), sd=synth.vgg19_state_dict, content=content, styles=[style], init=init,
                guides=guides, size=64)


def vgg40x56():
    gen = torch.Generator().manual_seed(11)
    content = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    s1 = torch.rand(1, 3, 48, 48, generator=gen) * 255 - 120
    s2 = torch.rand(1, 3, 36, 60, generator=gen) * 255 - 120
    init = torch.rand(1, 3, 40, 56, generator=gen) * 255 - 120
    g2 = torch.zeros(3, 36, 60)
    g2[0, :, :24], g2[1, :, 24:] = 1, 1  # region 2 is absent from the second style image
    guides = (halves(3, 40, 56), [halves(3, 48, 48, vertical=False), g2])
    return dict(cfg=make_cfg(style_blend_weights=[0.25, 0.75]), flags=["--style_blend_weights", "0.3,0.9"], kw=dict(S=56, styles=("s1.png", "s2.png")),
                sd=synth.vgg19_state_dict, content=content, styles=[s1, s2], init=init, guides=guides, size=56)


def nin99():
    content, style, init = synth.images(99)
    soft = torch.rand(2, 99, 99, generator=torch.Generator().manual_seed(3))
    return dict(cfg=make_cfg(use_covariance=True, **NIN_LAYERS), flags=NIN_FLAGS + ["--use_covariance"], kw=dict(model="nin", S=99),
                sd=synth.nin_state_dict, content=content, styles=[style], init=init, guides=(halves(2, 99, 99), [soft]), size=99)


CONFIGS = {
    "vgg19-64-two-regions": vgg64,
    "vgg19-40x56-two-styles-three-regions": vgg40x56,
    "nin-99-covariance-soft": nin99,
    "vgg19-64-no-grad-norm": lambda: vgg64(["--no_grad_norm"], normalize_gradients=False),
    "vgg19-64-vsf-0": lambda: vgg64(["--video_style_factor", "0"], video_style_factor=0.0),
}


def compare(name, slots, total, grad, slots_r, total_r, grad_r):
    for k, (a, b) in enumerate(zip(slots, slots_r)):
        print(f"  {name} slot {k}: {a:.9e} ({b:.9e})")
        assert abs(a - b) <= TOL_LOSS * abs(b), (name, k, a, b)
    assert abs(total - total_r) <= TOL_LOSS * abs(total_r), (name, total, total_r)
    e = rel_l2(grad, grad_r)
    print(f"  {name}: pixel gradient rel-L2 {e:.3e}")
    assert e <= TOL_GRAD, (name, e)


@pytest.mark.parametrize("config", list(CONFIGS), ids=list(CONFIGS))
def test_evaluation_against_fp64_and_the_module_path(weight_files, config):
    from oracle.style_oracle import loss_order
    p = CONFIGS[config]()
    sd = p["sd"](dtype=torch.float64)
    ref = gr.build(p["content"].double(), [s.double() for s in p["styles"]], p["cfg"], sd, p["guides"])
    total_r, losses_r, grad_r = ref.feval(p["init"].double(), p["guides"][0])
    args = product_args(weight_files, p["flags"], **p["kw"])
    net, losses, opt = prepared(args, p["content"], p["styles"], p["init"], p["guides"], p["size"])
    slots, total, grad = opt.feval()
    torch.cuda.synchronize()
    assert opt.engine is not None, "the guided network left the engine"
    assert all(id(s) in opt.engine.guided for s in opt.engine.steps if s.kind == "style")
    assert not opt.engine.fused_gram and not opt.engine.image_gram, "a whole-plane fusion was planned for a guided layer"
    got = (slots.cpu().double().tolist(), float(total), grad.cpu().clone())
    order = loss_order(ref.spec)
    assert len(order) == len(losses)
    want = [float(losses_r[i]) if i in losses_r else 0.0 for i in order]
    compare("engine vs fp64", got[0], got[1], got[2], want, float(total_r), grad_r)
    slots_m, total_m, grad_m = opt._feval_modules()
    torch.cuda.synchronize()
    compare("engine vs module path", got[0], got[1], got[2], slots_m.cpu().double().tolist(), float(total_m), grad_m.cpu())


def test_all_ones_guides_match_the_unguided_engine(weight_files):
    content, style, init = synth.images(64)
    ones = (torch.ones(1, 64, 64), [torch.ones(1, 64, 64)])
    net, losses, opt = prepared(product_args(weight_files, S=64), content, [style], init, None, 64)
    slots_u, total_u, grad_u = opt.feval()
    assert opt.engine is not None and not opt.engine.guided
    want = (slots_u.cpu().double().tolist(), float(total_u), grad_u.cpu().clone())
    net, losses, opt = prepared(product_args(weight_files, S=64), content, [style], init, ones, 64)
    slots_g, total_g, grad_g = opt.feval()
    torch.cuda.synchronize()
    assert opt.engine is not None and opt.engine.guided
    compare("guided (all ones) vs unguided engine", slots_g.cpu().double().tolist(), float(total_g), grad_g.cpu(), *want)


_REFS = {}


def trajectory_refs(opt_name):
    if opt_name not in _REFS:
        cfg = make_cfg(optimizer=opt_name)
        content, style, init = synth.images(64)
        guides = (halves(2, 64, 64), [halves(2, 64, 64, vertical=False)])
        ref64 = gr.optimize(content.double(), [style.double()], init.double(), 5, cfg, synth.vgg19_state_dict(dtype=torch.float64), guides, torch.float64)
        ref32 = gr.optimize(content, [style], init, 5, cfg, synth.vgg19_state_dict(), guides, torch.float32)
        _REFS[opt_name] = (content, style, init, guides, ref64, ref32)
    return _REFS[opt_name]


def five_iterations(weight_files, opt_name, hip_graph):
    import optim
    content, style, init, guides, ref64, ref32 = trajectory_refs(opt_name)
    args = product_args(weight_files, optimizer=opt_name, S=64, N=5)
    args.hip_graph = hip_graph
    out = optim.optimize(content, [style], init.clone(), 5, args, guides=guides)
    assert out.shape == init.shape and out.dtype == torch.float32 and not out.is_cuda
    floor, err = rel_l2(ref32, ref64), rel_l2(out, ref64)
    print(f"{opt_name} (hip_graph={hip_graph}): relL2(ours, f64) {err:.3e}, relL2(restatement in fp32, f64) {floor:.3e}")
    assert err <= max(1e-3, 2 * floor), (err, floor)
    assert rel_l2(out, init) > 1e-3  # (it moved)
    return out


def test_five_lbfgs_iterations_graph_and_eager(weight_files, monkeypatch):
    import optim
    engines = []
    keep = optim.PixelOptimizer.step

    def step(self):
        engines.append((self.engine is not None, self._graph is not None))
        return keep(self)

    monkeypatch.setattr(optim.PixelOptimizer, "step", step)
    graph = five_iterations(weight_files, "lbfgs", 1)
    assert all(e for e, _ in engines) and any(g for _, g in engines), "the guided job did not replay a captured L-BFGS iteration"
    del engines[:]
    eager = five_iterations(weight_files, "lbfgs", 0)
    assert all(e for e, _ in engines) and not any(g for _, g in engines)
    assert torch.equal(graph, eager), "captured graph and eager launches disagree"


def test_five_adam_steps(weight_files):
    five_iterations(weight_files, "adam", 0)


def test_plan_follows_the_guides_from_call_to_call(weight_files):
    """One network: unguided, guided, guided with other content guides, unguided - each call bit-equal to the same call on a fresh network
    (the whole-plane fusions come back, none leaks into a guided plan, no captured iteration outlives its guides)."""
    import models
    import optim
    content, style, init = synth.images(64)
    g1 = (halves(2, 64, 64), [halves(2, 64, 64, vertical=False)])
    g2 = (halves(2, 64, 64, vertical=False), [halves(2, 64, 64, vertical=False)])

    def network():
        args = product_args(weight_files, S=64, N=3)
        args.hip_graph, args._maua_repeated_calls = 1, True  # (iterations captured as bundles that the next call on the network may replay)
        optim.set_model_args(args, 64)
        return (args,) + tuple(models.load_model(args))

    def run(n, guides):
        args, net, losses = n
        out = optim.optimize(content, [style], init.clone(), 3, args, net=net, losses=losses, guides=guides)
        eng = net._maua_engine
        assert bool(eng.guided) == (guides is not None) and not (guides is not None and (eng.fused_gram or eng.image_gram))
        return out

    shared = network()
    first, guided1, guided2, third = run(shared, None), run(shared, g1), run(shared, g2), run(shared, None)
    assert torch.equal(third, first), "the unguided plan did not come back"
    assert torch.equal(guided1, run(network(), g1)), "a guided call depends on what the network ran before"
    assert torch.equal(guided2, run(network(), g2)), "new content guides: a stale plan or graph was served"
    assert not torch.equal(guided1, guided2) and not torch.equal(guided1, first)


def test_debug_poison_changes_nothing(weight_files, monkeypatch):
    import plan
    p = vgg64()
    results = []
    for poison in ("0", "1"):
        monkeypatch.setitem(plan.OVERRIDES, "debug_poison", poison)
        net, losses, opt = prepared(product_args(weight_files, S=64), p["content"], p["styles"], p["init"], p["guides"], 64)
        slots, total, grad = opt.feval()
        torch.cuda.synchronize()
        assert opt.engine is not None and opt.engine.guided
        results.append((slots.cpu().clone(), total.cpu().clone(), grad.cpu().clone()))
    for a, b in zip(*results):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


def test_field_off_keeps_the_module_path(weight_files, monkeypatch):
    import plan
    monkeypatch.setitem(plan.OVERRIDES, "guided_engine", "0")
    p = vgg64()
    net, losses, opt = prepared(product_args(weight_files, S=64), p["content"], p["styles"], p["init"], p["guides"], 64)
    opt.feval()
    assert opt.engine is None
