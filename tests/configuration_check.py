"""One function evaluation of the fused engine against the CPU oracle (oracle/style_oracle.py), shared by
tests/test_random_shapes_gpu.py (random configurations under the default plan) and tests/test_plan_variants_gpu.py (fixed configurations
under every alternative plan).

Bars: every module's loss 1e-4 of the fp64 oracle (the bar of test_engine_feval_matches_reference).  The engine's decisions - ReLU
masks, max-pool arg-maxes (tests/engine_decisions.py) - pin a second fp64 evaluation, which then differs from the engine by arithmetic
alone: every materialised activation 2e-6 of the pinned forward, the pixel gradient 1e-4 rel-L2 of the pinned gradient, whatever the
decisions.  Unpinned, a decision within rounding of its boundary can fall on the other side than in fp64 (at
S = 151 with avg pooling ONE relu2_1 activation of 720 000 is 0 here and 2.7e-5 in fp64 and moves the image gradient by 1.6e-3): the
unpinned gradient is held to 1e-4 when the engine takes every decision as fp64 does, and the number of decisions it takes otherwise
is bounded by the fp32 oracle's on the same inputs.

`oracle_reference` is the part that does not depend on the engine (the unpinned fp64 and fp32 oracle evaluations): a caller that evaluates
one configuration under several plans computes it once.  `check_configuration` evaluates, reads the decisions, runs the pinned fp64 pass,
asserts the bars and returns what it measured."""
import os

import torch

from conftest import rel_l2
from engine_decisions import FLIP_FACTOR, FLIP_SLACK, activation_map, count_flips, engine_decisions, oracle_decisions

ACT_BAR = 2e-6   # a materialised activation of a split-precision layer (fp16x3 / bf16x6) against the pinned fp64 forward


class _Threads:
    """The oracle on up to 16 host threads (fp64 and the decision counts do not depend on the count)."""

    def __enter__(self):
        self.before = torch.get_num_threads()
        torch.set_num_threads(min(16, os.cpu_count() or 1))

    def __exit__(self, *exc):
        torch.set_num_threads(self.before)


def oracle_reference(args, sd, content, style_images, init, keep_fp32_activations=False):
    """The oracle's own evaluations of a configuration: fp64 (losses, gradient, activations, decisions) and the fp32 oracle's count of
    decisions taken differently from fp64.  `keep_fp32_activations`: the fp32 forward's activations stay in the result (`acts32`) for
    callers that set a bar from the fp32 oracle's distance."""
    from oracle import OracleNet, build_spec
    with _Threads():
        nets = {}
        for dt in (torch.float64, torch.float32):
            onet = OracleNet(build_spec(args), sd, dtype=dt)
            onet.capture_content(content)
            onet.capture_style(style_images, args.style_blend_weights)
            if args.normalize_weights:
                onet.normalize_weights()
            nets[dt] = onet
        onet = nets[torch.float64]
        spec = onet.spec
        ototal, olosses, ograd = onet.feval(init)
        acts, aux = onet._forward(init.double())
        acts32, aux32 = nets[torch.float32]._forward(init.float())
        o_flips = count_flips(spec, oracle_decisions(spec, acts32, aux32), acts, aux)
    ref = dict(onet=onet, spec=spec, ototal=ototal, olosses=olosses, ograd=ograd, acts=acts, aux=aux, o_flips=o_flips)
    if keep_fp32_activations:
        ref["acts32"] = acts32
    return ref


def check_configuration(label, tag, args, net, opt, content, style_images, init, sd, reference=None, fp32_activations=()):
    """Evaluate `opt` (an optim.PixelOptimizer built on `net` for `args`, B = 1) once and hold it to the bars of the module docstring.
    `label` heads the printed line, `tag` goes into every assertion message.  `reference`: oracle_reference's result for this
    configuration (computed here when None).  `fp32_activations`: engine activation indices whose layer runs an fp32 kernel (fp32
    matrix cores / direct): their bar is twice the distance of the fp32 oracle's activation from the pinned fp64 forward, at least
    ACT_BAR (needs `acts32` in the reference); both numbers are printed.
    Returns the measured numbers: losses [(name, engine, fp64)], activations {index: (error, bar)}, fp32_distance {index: d}, pinned and
    unpinned gradient error, engine_flips, oracle_flips, and the engine's slots / total / gradient on the host."""
    from oracle.style_oracle import loss_order
    slots, total, grad = opt.feval()
    torch.cuda.synchronize()
    slots, total, grad = slots.clone().cpu(), total.clone().cpu(), grad.clone().cpu()
    assert opt.engine is not None, (*tag, "evaluated off the fused engine: no decisions to read")
    ref = reference if reference is not None else oracle_reference(args, sd, content, style_images, init, bool(fp32_activations))
    onet, spec, acts, aux = ref["onet"], ref["spec"], ref["acts"], ref["aux"]
    with _Threads():
        decisions, e_flips = engine_decisions(opt.engine, spec, acts, aux)
        pacts, _ = onet._forward(init.double(), decisions=decisions)
        _, _, pgrad = onet.feval(init, decisions=decisions)
    o_flips, olosses, ograd = ref["o_flips"], ref["olosses"], ref["ograd"]
    order = loss_order(spec)
    got = slots.tolist()
    losses = []
    for k, i in enumerate(order):
        want = float(olosses.get(i, 0.0))
        losses.append((spec[i].name, got[k], want))
        assert abs(got[k] - want) <= 1e-4 * max(abs(want), 1e-9), (*tag, spec[i].name, got[k], want)
    checked, activations, fp32_distance = 0, {}, {}
    for k, i in activation_map(opt.engine, spec).items():
        v = opt.engine.act[k]
        if v.is_meta:
            continue   # (pooled in the producing launch: only the pooled map exists)
        err = rel_l2(v.cpu(), pacts[i])
        bar = ACT_BAR
        if k in fp32_activations:
            fp32_distance[k] = rel_l2(ref["acts32"][i], pacts[i])
            bar = max(ACT_BAR, 2 * fp32_distance[k])
            print(f"{label}: activation {k} ({spec[i].name or spec[i].kind}) on an fp32 kernel: {err:.2e} of the pinned fp64 forward, "
                  f"fp32 oracle {fp32_distance[k]:.2e}, bar {bar:.2e}")
        activations[k] = (err, bar)
        assert err <= bar, (*tag, k, spec[i].kind, err)
        checked += 1
    assert checked > 0
    rel, pinned = rel_l2(grad, ograd), rel_l2(grad, pgrad)
    e, o = sum(e_flips.values()), sum(o_flips.values())
    print(f"{label}: gradient {rel:.2e} unpinned, {pinned:.2e} pinned; decisions off fp64: engine {e}, fp32 oracle {o}")
    assert pinned <= 1e-4, (*tag, pinned, rel, e)
    assert e <= FLIP_FACTOR * o + FLIP_SLACK, (*tag, e, o, {spec[i].name or i: n for i, n in e_flips.items() if n})
    if e == 0:
        assert rel <= 1e-4, (*tag, rel)
    return dict(losses=losses, activations=activations, fp32_distance=fp32_distance, pinned=pinned, unpinned=rel, engine_flips=e, oracle_flips=o,
                slots=slots, total=total, grad=grad)
