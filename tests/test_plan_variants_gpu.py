"""Every HOST field of the planner (the "host" entries of plan.FIELDS: the switches models.py, engine.py and optim.py read, what
MAUA_PLAN="field=value" sets and tools/ab_*.sh compare) at its NON-default values, through the whole engine.

The kernels behind these switches are tested one by one; what nothing evaluated is the engine's plumbing around them under each
alternative plan - which buffer is a meta tensor, which mask is applied by whom, which workspace a side stream owns, which slot a loss
lands in.  `HOST_VARIANTS` lists the values this module evaluates the engine under, `HOST_COVERED_ELSEWHERE` the fields an existing test
forces already; tests/test_host_logic.py checks that the two tables cover plan.FIELDS (a host field added later without a test of its
other setting fails there), so this module imports without a GPU.

How a field is forced: plan.OVERRIDES[field] = value, in-process, BEFORE models.load_model / StyleEngine / PixelOptimizer are built (the
plan is read when the engine is built and when it prepares its buffers); an autouse fixture removes what a test set.

Configurations (seeded: synth.images, conftest.product_args; as small as the routes allow):
  V   VGG-19, one image, S = 72: style losses on relu1_1, relu2_1, relu3_1, relu4_1, content loss on relu4_2, TV, max pooling.  Planes of
      72, 36, 18 and 9 pixels a side (ragged 16 x 32 and 8-row tiles, the odd 9 x 9 plane behind a floor-mode pool), consumed channel
      counts 3, 64, 128, 256, 512: every family's channel threshold and every fused group occurs once.
  Vc  V with avg pooling and --use_covariance (the Gram / loss chain's other form).
  N   NIN at S = 150 (the smallest side draw_config of tests/test_random_shapes_gpu.py allows), covariance form: the strided stem, the
      1x1 and 5x5 layers, the 3x3 / 2 ceil-mode pools.
  W   three independent frames of S = 64 through optim's frame-batch path.
  G   four L-BFGS iterations at S = 32 through optim.optimize.

The wide kernel families are routed by default only on large launches (x3w_min_pixels = 4096 pixels, conv_x3q_preferred,
conv_x3p_preferred).  Where a variant needs them on these planes the test lowers x3w_min_pixels, x3q_min_fill, x3q_min_chunks, x3p_min_fill,
x3p_min_items (and forces x3p_ks = 1: the persistent kernel is only routed unsplit) - `LOW*` below - for the variant AND for the
baseline it is compared with; those constants' own non-default values are tested kernel by kernel in tests/test_tuning_variants_gpu.py.

Two kinds of field:
 (a) the field sends layers to other arithmetic: one evaluation against the CPU oracle under the bars of tests/configuration_check.py
     (losses 1e-4 of fp64, pinned gradient 1e-4, flips bounded by the fp32 oracle's, unpinned gradient 1e-4 without flips, materialised
     activations 2e-6 of the pinned fp64 forward) - except that an activation whose layer the variant moves to an fp32 kernel (fp32
     matrix cores / direct: `conv2d_fwd` in the route records, and the pool behind it) is held to twice the distance of the fp32 CPU
     oracle's activation from the same pinned fp64 forward, at least 2e-6: nobody had measured those against fp64, so no constant.
 (b) the alternative must leave every bit unchanged (include/maua_hip.h promises it for every launch that changes; for the stream and
     graph fields it follows from fixed-order reductions - a difference is a missing event wait or a shared workspace): torch.equal on
     loss slots, total and pixel gradient (G: the final image) against the baseline plan, the variant evaluated five times; the
     baseline itself is held to the bars of (a) once per configuration.
No variant is vacuous: (a) asserts on StyleEngine.describe_routes that the layers moved as the field says, (b) probes the engine's
structure.  Nothing is skipped.

Table (field: values, configuration, kind):
  conv_x6: 0 / fwd / bwd on V, 0 on N, (a)            conv_x3: 0 on V and N, (a)           conv_x3w: 0 on V [LOW], (a)
  conv_x3q: 0 and 64 on V [LOW, conv_x3p = 0 on both sides so that conv_x3q gets the layers], (a)
  conv_x3p: 0 and 256 on V [LOW + x3p_ks = 1], (a)     conv_x3p_max: 128, same, (a)         x3p_gram_min_mb: 0, same, (a)
  conv_image: 0 on V, (a)    split_min_produced: 1 on V (nothing of NIN produces fewer than 16 channels from a 3x3 layer), 1000000 on V and N, (a)
  x3w_min_pixels: 0 on V and N, 1000000000 on V (every plane of N at S = 150 is below the default already), (a)
  pool_codes: 0 on V, (b)    fuse_pool_split: 0 on V, (b)    finish_in_launch: 1 on V, (b)
  style_stream: 1 against 0 on V, (b); evaluated on a stream of its own beside a busy side stream, the Gram / D matrices set to NaN
      before (evaluate_beside_busy_side_streams), so that a consumer that does not wait for the side stream reads NaN
  loss_ledger, gram_batch, gram_partial_batch: 0 on Vc, (b); image_gram = 0 on both sides (each of the three drops the image layer's
      Gram slabs, which change rounding: test_gram_slabs_from_the_image_layer_change_nothing_but_rounding; moot under covariance, kept
      so that the pairing survives a change of the configuration)
  dmat_pack_batch: 0 on V with x3w_min_pixels = 0 on both sides, (b): under covariance no style layer's Gram backward is fused
      (engine._prepare), so Vc would pack nothing and the variant would be vacuous; on V three layers pack
  side_streams: 0 and 1 against 4 on W, (b), evaluated the same way            graph_bundles: 0 on G, (b)

Measured on an MI355X (every test prints its own numbers):
  (a) on V: pinned gradient 3.5e-7 ... 6.1e-7, worst materialised activation 4.8e-7 ... 7.4e-7, at most one decision off fp64 (the fp32
      oracle: one); unpinned = pinned without a flip, 1.06e-4 with the one flip of conv_x3 = 0.  On N: pinned gradient 1.8e-6 ... 2.8e-6,
      worst activation 4.1e-7 ... 6.4e-7, at most one decision off fp64 (the fp32 oracle: none).  Losses a few 1e-7 of fp64.
  activations on fp32 kernels (conv_x6 = 0 / bwd, split_min_produced = 1000000, NIN's 1x1 / 5x5 / stem under conv_x3 = 0 and by default):
      V 9.7e-8 (relu1_1) ... 7.4e-7 (relu4_2) where the fp32 oracle is 9.8e-8 ... 5.6e-7 from the same pinned forward; N 2.9e-7 ... 6.4e-7
      where the oracle is 3.1e-7 ... 6.5e-7.  Twice the oracle's distance stays below the floor, so the bar was 2e-6 everywhere.
  (b) every variant 5 / 5 evaluations bit-identical; baselines V 4.0e-7, Vc 2.5e-7, frame 0 of W alone 1.7e-6 (pinned gradient), G 8.3e-6
      of the fp64 trajectory after four iterations.
"""
import pytest
import torch

import plan
from conftest import NIN_FLAGS, product_args, rel_l2

pytestmark = pytest.mark.gpu

# field -> the non-default values this module evaluates the engine under (strings: what MAUA_PLAN would hold)
HOST_VARIANTS = {
    "conv_x6": ("0", "fwd", "bwd"),
    "conv_x3": ("0",),
    "conv_x3w": ("0",),
    "conv_x3q": ("0", "64"),
    "conv_x3p": ("0", "256"),
    "conv_x3p_max": ("128",),
    "x3p_gram_min_mb": ("0",),
    "conv_image": ("0",),
    "split_min_produced": ("1", "1000000"),
    "x3w_min_pixels": ("0", "1000000000"),
    "pool_codes": ("0",),
    "loss_ledger": ("0",),
    "gram_batch": ("0",),
    "gram_partial_batch": ("0",),
    "fuse_pool_split": ("0",),
    "dmat_pack_batch": ("0",),
    "finish_in_launch": ("1",),
    "style_stream": ("1",),
    "side_streams": ("0", "1"),
    "graph_bundles": ("0",),
}
# field -> an existing test that forces it through the engine (or, frame_cache_mb: the host structure it sizes)
HOST_COVERED_ELSEWHERE = {
    "fuse_pool": "tests/test_engine_gpu.py::test_pool_in_the_convolution_epilogue_changes_no_bit",
    "fuse_unpool": "tests/test_engine_gpu.py::test_pool_backward_in_the_convolution_staging_changes_no_bit",
    "fuse_gram_max_c": "tests/test_engine_gpu.py::test_gram_backward_fused_into_the_convolution_equals_the_separate_pass",
    "image_gram": "tests/test_engine_gpu.py::test_gram_slabs_from_the_image_layer_change_nothing_but_rounding",
    "few_mfma": "tests/test_conv_few_mfma_gpu.py::test_engine_routes_the_image_layer_backward_and_matches_the_vector_kernel",
    "strided_fwd_3x3": "tests/test_strided_as_3x3_gpu.py::test_nin_engine_with_and_without_the_3x3_stem_against_the_fp64_oracle",
    "strided_bwd_3x3": "tests/test_strided_as_3x3_gpu.py::test_nin_engine_with_and_without_the_3x3_stem_against_the_fp64_oracle",
    "hip_graph": "tests/test_engine_gpu.py::test_iteration_graph_is_captured_once_per_network_and_changes_no_bit",
    "frame_batch": "tests/test_cli_gpu.py::test_vid_img_frame_batches_match_the_frame_by_frame_loop",
    "temporal_device": "tests/test_temporal_device_gpu.py::test_vid_img_with_flow_cache_on_the_device",
    "clip_device": "tests/test_clip_device_gpu.py::test_img_vid_with_the_clip_on_the_device",
    "guided_engine": "tests/test_guided_engine_gpu.py::test_field_off_keeps_the_module_path",
    "debug_poison": "tests/test_guided_engine_gpu.py::test_debug_poison_changes_nothing",
    "frame_cache_mb": "tests/test_host_logic.py::test_frame_cache_budget_holds_under_inserts_overwrites_and_pops",
}

# the wide families on small planes (module docstring): set for the variant and for its baseline
LOW = {"x3w_min_pixels": "0", "x3q_min_fill": "0", "x3q_min_chunks": "0", "x3p_min_fill": "0", "x3p_min_items": "0"}
LOWQ = dict(LOW, conv_x3p="0")    # ... conv_x3q gets the layers of 256 channels and more, conv_x3w the rest
LOWP = dict(LOW, x3p_ks="1")      # ... conv_x3p gets every layer of 64 channels and more

# (field, value) -> (configurations, what baseline and variant share)
KIND_A = {
    ("conv_x6", "0"): (("V", "N"), {}),
    ("conv_x6", "fwd"): (("V",), {}),
    ("conv_x6", "bwd"): (("V",), {}),
    ("conv_x3", "0"): (("V", "N"), {}),
    ("conv_x3w", "0"): (("V",), LOW),
    ("conv_x3q", "0"): (("V",), LOWQ),
    ("conv_x3q", "64"): (("V",), LOWQ),
    ("conv_x3p", "0"): (("V",), LOWP),
    ("conv_x3p", "256"): (("V",), LOWP),
    ("conv_x3p_max", "128"): (("V",), LOWP),
    ("x3p_gram_min_mb", "0"): (("V",), LOWP),
    ("conv_image", "0"): (("V",), {}),
    ("split_min_produced", "1"): (("V",), {}),
    ("split_min_produced", "1000000"): (("V", "N"), {}),
    ("x3w_min_pixels", "0"): (("V", "N"), {}),
    ("x3w_min_pixels", "1000000000"): (("V",), {}),
}
KIND_B = {
    ("pool_codes", "0"): ("V", {}),
    ("loss_ledger", "0"): ("Vc", {"image_gram": "0"}),
    ("gram_batch", "0"): ("Vc", {"image_gram": "0"}),
    ("gram_partial_batch", "0"): ("Vc", {"image_gram": "0"}),
    ("dmat_pack_batch", "0"): ("V", {"x3w_min_pixels": "0"}),
    ("fuse_pool_split", "0"): ("V", {}),
    ("finish_in_launch", "1"): ("V", {}),
    ("style_stream", "1"): ("V", {"style_stream": "0"}),
}
KIND_A_CASES = list(KIND_A)
KIND_B_CASES = list(KIND_B) + [("side_streams", "0"), ("side_streams", "1"), ("graph_bundles", "0")]

V_LAYERS = ["--style_layers", "relu1_1,relu2_1,relu3_1,relu4_1", "--content_layers", "relu4_2"]
CONFIGS = {
    "V": dict(model="vgg19", S=72, extra=V_LAYERS),
    "Vc": dict(model="vgg19", S=72, extra=V_LAYERS + ["--pooling", "avg", "--use_covariance"]),
    "N": dict(model="nin", S=150, extra=NIN_FLAGS + ["--use_covariance"]),
}

SPLIT3 = ("conv_x3", "conv_x3w", "conv_x3q", "conv_x3p")            # the fp16x3 3x3 families
WIDE = ("conv_x3w", "conv_x3q", "conv_x3p")
FP32 = ("conv2d_fwd", "conv2d_bwd_data", "conv3x3_few_out")         # the generic entry points: direct / fp32 matrix cores


@pytest.fixture(scope="module")
def hip():
    import hip as h
    h.lib()
    return h


@pytest.fixture(autouse=True)
def _restore(hip):
    yield
    plan.OVERRIDES.clear()
    plan.forward_to_library(hip.lib())
    hip.conv_arm_workspace(None)


def force(hip, fields):
    """Planner fields for everything built from here on (host fields are read at build / _prepare time, the library's at the launch)."""
    for k, v in fields.items():
        assert k in plan.FIELDS
        plan.OVERRIDES[k] = str(v)
    plan.forward_to_library(hip.lib())


class Built:
    """A configuration built under the plan in force: args, network, optimiser (B = 1) and the inputs the oracle needs."""

    def __init__(self, weight_files, config):
        import models
        import optim
        import synth
        cfg = CONFIGS[config]
        S = cfg["S"]
        self.config, self.S = config, S
        self.args = product_args(weight_files, cfg["extra"], model=cfg["model"], S=S, N=3)
        self.content, style, self.init = synth.images(S)
        self.styles = [style]
        self.sd = synth.nin_state_dict() if cfg["model"] == "nin" else synth.vgg19_state_dict()
        optim.set_model_args(self.args, S)
        self.net, self.losses = models.load_model(self.args)
        optim.set_content_targets(self.net, self.content, self.args)
        optim.set_style_targets(self.net, self.styles, self.args)
        for m in self.losses:
            m.mode = "loss"
        self.opt = optim.PixelOptimizer(self.net, self.losses, self.init, self.args)
        assert self.opt.engine is not None
        self.engine = self.opt.engine

    def evaluate(self):
        slots, total, grad = evaluate_beside_busy_side_streams(self.engine, self.opt.feval)
        torch.cuda.synchronize()
        return slots.clone().cpu(), total.clone().cpu(), grad.clone().cpu()

    def check(self, label, references, fp32_activations=()):
        from configuration_check import check_configuration
        m = check_configuration(label, (label,), self.args, self.net, self.opt, self.content, self.styles, self.init, self.sd,
                                reference=references(self), fp32_activations=fp32_activations)
        print(f"{label}: losses " + ", ".join(f"{n} {g:.6e} (fp64 {w:.6e})" for n, g, w in m["losses"]))
        print(f"{label}: worst activation {max(e for e, _ in m['activations'].values()):.2e}")
        return m


@pytest.fixture(scope="module")
def references():
    """The oracle's unpinned fp64 and fp32 evaluations, once per configuration: they do not depend on the plan."""
    from configuration_check import oracle_reference
    cache = {}

    def get(built):
        if built.config not in cache:
            cache[built.config] = oracle_reference(built.args, built.sd, built.content, built.styles, built.init, keep_fp32_activations=True)
        return cache[built.config]
    return get


@pytest.fixture(scope="module")
def baselines(hip, references):
    """(routes, engine, measured numbers) of a configuration under a baseline plan, evaluated - and held to the fp64 bars - once."""
    cache = {}

    def get(weight_files, config, shared):
        key = (config, tuple(sorted(shared.items())))
        if key not in cache:
            keep = dict(plan.OVERRIDES)
            plan.OVERRIDES.clear()
            force(hip, shared)
            b = Built(weight_files, config)
            routes = b.engine.describe_routes(b.opt.x)
            m = b.check(f"baseline {config} {dict(shared)}", references, fp32_forward(b.engine, routes))
            cache[key] = (routes, b.engine, m)
            plan.OVERRIDES.clear()
            force(hip, keep)
        return cache[key]
    return get


def fp32_forward(engine, routes):
    """Engine activation indices written by an fp32 kernel in the forward pass (`conv2d_fwd`: one forward record per conv step, in
    order), and the pooled maps behind them (a selection / average of the same values)."""
    convs = [s for s in engine.steps if s.kind == "conv"]
    fwd = [r for r in routes if r["pass"] == "fwd"]
    assert len(convs) == len(fwd)
    out = {s.dst for s, r in zip(convs, fwd) if r["kernel"] == "conv2d_fwd"}
    for s in engine.steps:
        if s.kind == "pool" and s.src in out:
            out.add(s.dst)
    return out


def by_pass(routes, which):
    return [r for r in routes if r["pass"] == which]


def kernels(routes, which):
    return [r["kernel"] for r in by_pass(routes, which)]


def moved(base, var, which, was, now):
    """The records of one pass whose kernel was among `was` in the baseline: each names one of `now` under the variant; their number."""
    pairs = [(b, v) for b, v in zip(by_pass(base, which), by_pass(var, which)) if b["kernel"] in was]
    for b, v in pairs:
        assert v["kernel"] in now, (which, b, v)
    return len(pairs)


def unchanged(base, var, which, but=()):
    for b, v in zip(by_pass(base, which), by_pass(var, which)):
        if b["kernel"] not in but:
            assert b["kernel"] == v["kernel"], (which, b, v)


def check_routes(field, value, config, base, var, engine):
    """The variant's route records against the baseline's: the layers moved as the field says (module docstring: no vacuous variants)."""
    assert len(by_pass(base, "fwd")) == len(by_pass(var, "fwd")) and len(by_pass(base, "bwd")) == len(by_pass(var, "bwd"))
    every = [r["kernel"] for r in var]
    split = SPLIT3 + ("conv_x6", "conv_image", "conv1x1_x3", "conv_kxk_x3", "conv_few_mfma")
    if field == "conv_x6":
        off = {"0": ("fwd", "bwd"), "fwd": ("bwd",), "bwd": ("fwd",)}[value]
        for which in ("fwd", "bwd"):
            assert any(k in split for k in kernels(base, which))
            if which in off:   # the fp32 route in this pass: no split-precision family, no fused group
                assert all(k in FP32 for k in kernels(var, which)), kernels(var, which)
                assert not any(r.get("pool") or r.get("unpool") or r.get("gram") for r in by_pass(var, which))
            else:              # the split families, layer by layer as in the baseline
                assert kernels(var, which) == kernels(base, which) and any(k in SPLIT3 for k in kernels(var, which))
    elif field == "conv_x3":
        assert not any(k in SPLIT3 + ("conv1x1_x3", "conv_kxk_x3") for k in every), every
        for which in ("fwd", "bwd"):
            plain = [(b, v) for b, v in zip(by_pass(base, which), by_pass(var, which)) if b["kernel"] in SPLIT3 and not b.get("strided_as_3x3")]
            assert plain and all(v["kernel"] == "conv_x6" for _, v in plain), (which, plain)
            others = moved(base, var, which, ("conv1x1_x3", "conv_kxk_x3"), FP32)   # (NIN's 1x1 and 5x5 layers: the fp32 matrix cores)
            assert others > 0 or config != "N"
            unchanged(base, var, which, but=SPLIT3 + ("conv1x1_x3", "conv_kxk_x3"))
    elif field == "conv_x3w":
        assert not any(k in WIDE for k in every), every
        assert {"conv_x3w", "conv_x3q", "conv_x3p"} <= set(r["kernel"] for r in base)
        for which in ("fwd", "bwd"):
            assert moved(base, var, which, WIDE, ("conv_x3",)) > 0
            unchanged(base, var, which, but=WIDE)
    elif field == "conv_x3q" and value == "0":
        assert "conv_x3q" not in every
        for which in ("fwd", "bwd"):
            assert moved(base, var, which, ("conv_x3q",), ("conv_x3w",)) > 0
            unchanged(base, var, which, but=("conv_x3q",))
    elif field == "conv_x3q":
        for which in ("fwd", "bwd"):
            n = 0
            for b, v in zip(by_pass(base, which), by_pass(var, which)):
                if b["kernel"] not in SPLIT3:
                    assert v["kernel"] == b["kernel"]
                    continue
                assert b["consumed"] >= 64 and b["consumed"] % 32 == 0
                if v.get("gram"):                       # the Gram backward rides in conv_x3w's (or conv_x3p's) launch only
                    want = "conv_x3w"
                elif v.get("unpool"):                   # the unpooling form pays from 512 channels (models.X3Q_UNPOOL_MIN_CHANNELS)
                    want = "conv_x3q" if b["consumed"] >= 512 else "conv_x3w"
                else:
                    want = "conv_x3q"
                assert v["kernel"] == want, (which, b, v)
                n += b["kernel"] == "conv_x3w" and want == "conv_x3q"
            assert n > 0, which
    elif field == "conv_x3p" and value == "0":
        assert "conv_x3p" not in every
        for which in ("fwd", "bwd"):
            assert moved(base, var, which, ("conv_x3p",), ("conv_x3w", "conv_x3q")) > 0
            unchanged(base, var, which, but=("conv_x3p",))
    elif field in ("conv_x3p", "conv_x3p_max"):
        keeps = (lambda c: c >= 256) if field == "conv_x3p" else (lambda c: c <= 128)
        for which in ("fwd", "bwd"):
            kept = lost = 0
            for b, v in zip(by_pass(base, which), by_pass(var, which)):
                if b["kernel"] != "conv_x3p":
                    assert v["kernel"] == b["kernel"], (which, b, v)
                elif keeps(b["consumed"]):
                    assert v["kernel"] == "conv_x3p", (which, b, v)
                    kept += 1
                else:
                    assert v["kernel"] in ("conv_x3w", "conv_x3q"), (which, b, v)
                    lost += 1
            assert kept > 0 and lost > 0, (which, kept, lost)
    elif field == "x3p_gram_min_mb":
        bg, vg = [r for r in base if r.get("gram")], [r for r in var if r.get("gram")]
        assert len(bg) == len(vg) >= 2 and all(r["kernel"] == "conv_x3w" for r in bg), bg
        assert all(r["kernel"] == "conv_x3p" for r in vg), vg
        assert kernels(var, "fwd") == kernels(base, "fwd") and "conv_x3p" in kernels(base, "fwd")
        unchanged(base, [dict(r, kernel="conv_x3w") if r.get("gram") else r for r in var], "bwd")
    elif field == "conv_image":
        assert kernels(base, "fwd")[0] == "conv_image" and "conv_image" not in every
        assert by_pass(var, "fwd")[0]["kernel"] == "conv_x6" and by_pass(var, "fwd")[0]["consumed"] == 3
        unchanged(base, var, "fwd", but=("conv_image",))
        assert kernels(var, "bwd") == kernels(base, "bwd") and any(k in SPLIT3 for k in kernels(var, "bwd"))
    elif field == "split_min_produced" and value == "1":
        few_b, few_v = [r for r in base if r["produced"] <= 4], [r for r in var if r["produced"] <= 4]
        assert [r["kernel"] for r in few_b] == ["conv_few_mfma"] and len(few_v) == 1 and few_v[0]["kernel"] in SPLIT3 and few_v[0]["pass"] == "bwd", (few_b, few_v)
        assert kernels(var, "fwd") == kernels(base, "fwd") and any(k in SPLIT3 for k in kernels(var, "fwd"))
        unchanged(base, var, "bwd", but=("conv_few_mfma",))
    elif field == "split_min_produced":
        for which in ("fwd", "bwd"):
            three = [(b, v) for b, v in zip(by_pass(base, which), by_pass(var, which))
                     if b["kernel"] in SPLIT3 + ("conv_image", "conv_x6") and not b.get("strided_as_3x3")]
            assert three and all(v["kernel"] in FP32 for _, v in three), (which, three)
            unchanged(base, var, which, but=SPLIT3 + ("conv_image", "conv_x6"))
        assert not any(k in SPLIT3 + ("conv_image", "conv_x6") for k in every), every
    elif field == "x3w_min_pixels" and value == "0":
        assert "conv_x3" not in every
        for which in ("fwd", "bwd"):
            assert moved(base, var, which, ("conv_x3",), WIDE) > 0 and "conv_x3w" in kernels(var, which)
            if config == "N":   # the strided stem's plane of sites is large enough now: a 3x3 convolution over sites in both passes
                assert not any(r.get("strided_as_3x3") for r in by_pass(base, which)) and any(r.get("strided_as_3x3") for r in by_pass(var, which))
    elif field == "x3w_min_pixels":
        assert not any(k in WIDE for k in every), every
        for which in ("fwd", "bwd"):
            assert moved(base, var, which, WIDE, ("conv_x3",)) > 0
            unchanged(base, var, which, but=WIDE)
        assert not engine.fused_pool and not engine.fused_unpool and not engine.fused_gram
    else:
        raise AssertionError(f"no route expectation for {field}")


A_PARAMS = [(f, v, c) for (f, v), (configs, _) in KIND_A.items() for c in configs]


@pytest.mark.parametrize("field,value,config", A_PARAMS, ids=[f"{f}={v}-{c}" for f, v, c in A_PARAMS])
def test_fields_that_move_layers_to_other_kernels_against_fp64(hip, weight_files, references, baselines, field, value, config):
    """Kind (a) of the module docstring: the engine evaluated under the variant, its route records against the baseline's, its losses,
    activations, decisions and gradients against the CPU oracle."""
    shared = KIND_A[(field, value)][1]
    base_routes, _, _ = baselines(weight_files, config, shared)
    force(hip, dict(shared, **{field: value}))
    b = Built(weight_files, config)
    routes = b.engine.describe_routes(b.opt.x)
    for r in routes:
        print(f"{field}={value} {config}: {r}")
    check_routes(field, value, config, base_routes, routes, b.engine)
    b.check(f"{field}={value} on {config}", references, fp32_forward(b.engine, routes))


_busy = {}


def evaluate_beside_busy_side_streams(engine, evaluate):
    """One evaluation in which only the engine's own event waits order its streams.  Torch's default stream is the legacy one, which
    the runtime orders against every other stream by itself: an evaluation issued there is right even without the join in front of the
    backward pass (checked by hand: dropping it went unnoticed five times out of five) - while the product's captured iterations run
    on a capture stream, where the fork / join events are all there is.  So, for an engine with side streams: the evaluation is issued
    on a stream of its own; in front of it the Gram and D matrices of the style layers are filled with NaN and every side stream gets
    a one-wave kernel that spins for about 5 ms (torch.cuda._sleep, calibrated once; an evaluation takes about one millisecond, and
    a delay that fills the chip - matrix products - holds the main stream's kernels back just as long), so that the side streams'
    Gram / loss chains start late and a consumer that does not wait for them reads NaN (and finds no ledger record)."""
    if not engine.side:
        return evaluate()
    if not _busy:
        _busy["main"] = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(1000000)
        e1.record()
        torch.cuda.synchronize()
        _busy["cycles"] = int(1000000 * 5.0 / max(e0.elapsed_time(e1), 1e-3))
        print(f"a spin of 1e6 cycles takes {e0.elapsed_time(e1):.3f} ms: {_busy['cycles']} cycles in front of every side stream's work")
    for t in list(engine.gram.values()) + list(engine.dmat.values()):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    for st in engine.side:
        with torch.cuda.stream(st):
            torch.cuda._sleep(_busy["cycles"])
    with torch.cuda.stream(_busy["main"]):
        out = evaluate()
    torch.cuda.synchronize()
    return out


def probe(field, base, var):
    """Kind (b): the engine's structure shows that the alternative was built (and the baseline's that the default was)."""
    import models
    if field == "pool_codes":
        assert base.pool_codes and base.fused_pool and base.fused_unpool
        assert var.pool_codes == {} and not var.fused_pool and not var.fused_unpool
    elif field == "loss_ledger":
        assert base.ledger is not None and var.ledger is None
    elif field == "gram_batch":
        assert base.gram_batch_on is True and var.gram_batch_on is False
    elif field == "gram_partial_batch":
        assert base.gram_partial_batch_on is True and var.gram_partial_batch_on is False and var.gram_batch_on is True
    elif field == "dmat_pack_batch":
        assert len(base.fused_style) >= 2 and len(var.fused_style) == len(base.fused_style)
        assert ("pack", 0) in base._gram_batches and not any(isinstance(k, tuple) and k[0] == "pack" for k in var._gram_batches)
    elif field == "fuse_pool_split":
        def splits(eng, s):
            return models.conv3x3_fwd_family(s.mod, 1, *eng.act[s.src].shape[2:])[1]
        fb = [s for s in base.steps if id(s) in base.fused_pool]
        fv = [s for s in var.steps if id(s) in var.fused_pool]
        assert any(splits(base, s) > 1 for s in fb), "no conv + pool group of the baseline splits its channel loop"
        assert all(splits(var, s) == 1 for s in fv) and len(fv) == sum(1 for s in fb if splits(base, s) == 1) < len(fb)
    elif field == "finish_in_launch":
        assert base.ws_counters is None and var.ws_counters is not None
    elif field == "style_stream":
        assert len(base.side) == 0 and not base.style_aside and len(var.side) == 1 and var.style_aside
    else:
        raise AssertionError(f"no probe for {field}")


B_PARAMS = [(f, v) for f, v in KIND_B]


@pytest.mark.parametrize("field,value", B_PARAMS, ids=[f"{f}={v}" for f, v in B_PARAMS])
def test_fields_that_must_leave_every_bit_unchanged(hip, weight_files, references, baselines, field, value):
    """Kind (b) of the module docstring: loss slots, total and pixel gradient of the variant, evaluated five times, carry the bits of the
    baseline plan (itself held to the fp64 bars)."""
    config, shared = KIND_B[(field, value)]
    _, base_engine, base = baselines(weight_files, config, shared)
    force(hip, dict(shared, **{field: value}))
    b = Built(weight_files, config)
    for k in range(5):
        slots, total, grad = b.evaluate()
        if k == 0:
            probe(field, base_engine, b.engine)
        print(f"{field}={value} on {config}, evaluation {k}: slots {slots.tolist()} (baseline {base['slots'].tolist()}), total {float(total):.9e} "
              f"(baseline {float(base['total']):.9e}), gradient {rel_l2(grad, base['grad'].double()):.2e} from the baseline's")
        assert torch.isfinite(grad).all()
        assert torch.equal(slots, base["slots"]), (field, k)
        assert torch.equal(total, base["total"]), (field, k)
        assert torch.equal(grad, base["grad"]), (field, k)


# ------------------------------------------------------------------------------------------------------------------------------------
# W: independent frames on side streams
# ------------------------------------------------------------------------------------------------------------------------------------
W_S, W_B, W_N = 64, 3, 4


def frames_inputs():
    import synth
    style = synth.images(W_S)[1]
    contents = torch.cat([synth.images(W_S, seed=50 + k)[0] for k in range(W_B)])
    inits = torch.cat([synth.images(W_S, seed=60 + k)[2] for k in range(W_B)])
    return style, contents, inits


def frames_run(weight_files, evaluations):
    """optim.optimize_frames on W, then `evaluations` evaluations of the batch at the initial images on the same engine."""
    import models
    import optim
    style, contents, inits = frames_inputs()
    args = product_args(weight_files, optimizer="lbfgs", S=W_S, N=W_N)
    optim.set_model_args(args, W_S)
    net, losses = models.load_model(args)
    out = optim.optimize_frames(contents.cuda(), [style], inits.cuda(), W_N, args, net, losses).cpu()
    eng = net._maua_engine
    assert eng.independent and eng.batch_hint == W_B
    x = inits.cuda()
    evals = []
    for _ in range(evaluations):
        slots, total, grad = evaluate_beside_busy_side_streams(eng, lambda: eng.feval(x))
        torch.cuda.synchronize()
        evals.append((slots.clone().cpu(), total.clone().cpu(), grad.clone().cpu()))
    return dict(out=out, evals=evals, engine=eng, args=args, net=net, losses=losses)


@pytest.fixture(scope="module")
def frames_baseline(hip, weight_files):
    """W under the default plan (four side streams planned, three used), and its frame 0 alone - the same bits, tests/test_engine_gpu.py -
    against the fp64 bars."""
    import optim
    import synth
    from configuration_check import check_configuration
    assert not plan.OVERRIDES
    run = frames_run(weight_files, 1)
    assert len(run["engine"].side) == min(W_B, int(plan.FIELDS["side_streams"][0]))
    style, contents, inits = frames_inputs()
    args, net, losses = run["args"], run["net"], run["losses"]
    optim.set_content_targets(net, contents[0:1], args)
    for m in losses:
        m.mode = "loss"
    one = optim.PixelOptimizer(net, losses, inits[0:1], args, batch_hint=W_B)
    m = check_configuration("baseline W, frame 0 alone", ("W",), args, net, one, contents[0:1], [style], inits[0:1], synth.vgg19_state_dict())
    slots, total, grad = run["evals"][0]
    assert torch.equal(m["grad"][0], grad[0]) and torch.equal(m["slots"].flatten(), slots[0].flatten()) and torch.equal(m["total"].flatten(), total[0:1])
    return run


@pytest.mark.parametrize("streams", [v for f, v in KIND_B_CASES if f == "side_streams"])
def test_side_streams_leave_every_bit_unchanged(hip, weight_files, frames_baseline, streams):
    """side_streams = 0 (everything on one stream, one workspace) and 1 (all frames on one side stream) against the default 4: the
    per-frame Gram / loss / L-BFGS kernels of independent frames share nothing, so the images after four iterations and five evaluations
    of the batch carry the same bits; a difference means a missing event wait or a workspace two streams share."""
    force(hip, {"side_streams": streams})
    run = frames_run(weight_files, 5)
    assert len(run["engine"].side) == min(W_B, int(streams)) and len(run["engine"].side_ws) == len(run["engine"].side)
    base = frames_baseline
    assert torch.equal(run["out"], base["out"]) and not torch.equal(run["out"][0], run["out"][1])
    for k, (slots, total, grad) in enumerate(run["evals"]):
        print(f"side_streams={streams}, evaluation {k}: totals {total.tolist()} (baseline {base['evals'][0][1].tolist()})")
        assert torch.equal(slots, base["evals"][0][0]) and torch.equal(total, base["evals"][0][1]) and torch.equal(grad, base["evals"][0][2]), k


# ------------------------------------------------------------------------------------------------------------------------------------
# G: L-BFGS iterations replayed from a bundle kept on the engine, or captured by every call
# ------------------------------------------------------------------------------------------------------------------------------------
G_S, G_N = 32, 4


def lbfgs_calls(weight_files, calls):
    import models
    import optim
    import synth
    content, style, init = synth.images(G_S)
    args = product_args(weight_files, optimizer="lbfgs", S=G_S, N=G_N)
    args.hip_graph, args._maua_repeated_calls = 1, True   # (runs this short launch eagerly by default; a caller that announces repeats keeps bundles)
    optim.set_model_args(args, G_S)
    net, losses = models.load_model(args)
    outs = [optim.optimize(content, [style], init.clone(), G_N, args, net, losses) for _ in range(calls)]
    return outs, net._maua_engine, args


@pytest.mark.parametrize("value", [v for f, v in KIND_B_CASES if f == "graph_bundles"])
def test_graph_bundles_leave_every_bit_unchanged(hip, weight_files, value):
    """graph_bundles = 0: every call captures its own iteration graph and keeps nothing on the engine; the default keeps the captured
    iteration with its image and L-BFGS states and replays it from the second call on.  The image after four iterations is the same,
    bit for bit, five calls in a row; the baseline is held to the fp64 oracle's trajectory (1e-3, the bar of smoke())."""
    import synth
    from oracle import optimize as oracle_optimize
    base, eng, args = lbfgs_calls(weight_files, 2)
    assert len(eng.iter_graphs) == 1 and torch.equal(base[0], base[1])
    content, style, init = synth.images(G_S)
    ref = oracle_optimize(content, [style], init, G_N, args, synth.vgg19_state_dict(), dtype=torch.float64)
    err = rel_l2(base[0], ref)
    print(f"graph_bundles: baseline image after {G_N} iterations {err:.2e} of the fp64 oracle's")
    assert err <= 1e-3
    force(hip, {"graph_bundles": value})
    outs, eng, _ = lbfgs_calls(weight_files, 5)
    assert eng.iter_graphs == {}
    for k, out in enumerate(outs):
        assert torch.equal(out, base[0]), k
