"""Feature-histogram style loss without a GPU: the restatement (tests/feat_hist_restatement.py) - monotone and bounded matched values,
permutation of pixels, constant and all-zero channels, the last bin, its analytic gradient against autograd, factor 0 against the oracle's
evaluation, a factor changing every style layer and nothing else, the blend of two styles -, the binding table, the host-side argument
checks of the entry points, the documented sizes of state and workspace, the refusals of the modules and the preset keys on their way into
the modules."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import feat_hist_restatement as hr
import synth
from conftest import REPO, make_cfg, rel_l2

NAMES = ["maua_feat_hist_bwd", "maua_feat_hist_fwd", "maua_feat_hist_state_bytes", "maua_feat_hist_supported", "maua_feat_hist_workspace_bytes"]
PARAMS = [(16, 2), (256, 1024), (1024, 64)]


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


def maps(C=5, H=9, W=13, seed=1, hs=11, ws=17):
    """(working map relu(randn + 0.3), style map relu(2 randn + 1) of another plane size), float32 values held in fp64."""
    gen = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(2 * torch.randn(C, hs, ws, generator=gen) + 1)
    return f.double(), s.double()


def plan(c, n):
    """csrc/feat_hist.hip fh_plan: (chunks, chunk) of a channel's plane - about 2048 workgroups, chunks of whole 1024-element grains."""
    grains = -(-n // 1024)
    want = max(1, min(-(-2048 // c), grains))
    chunk = -(-(-(-n // want)) // 1024) * 1024
    return -(-n // chunk), chunk


@pytest.mark.parametrize("bins,knots", PARAMS)
def test_matched_values_are_monotone_in_f_and_inside_the_table(bins, knots):
    f, s = maps()
    table = hr.quantile_table(s, knots)
    assert bool((table[:, 1:] >= table[:, :-1]).all())
    r = hr.matched(f, table, bins).reshape(f.shape[0], -1)
    flat = f.reshape(f.shape[0], -1)
    for c in range(f.shape[0]):
        order = torch.argsort(flat[c], stable=True)
        assert bool((r[c][order][1:] >= r[c][order][:-1]).all()), c
        assert float(r[c].min()) >= float(table[c, 0]) and float(r[c].max()) <= float(table[c, -1]), c
        same = flat[c][order][1:] == flat[c][order][:-1]  # equal values get equal matched values: a tie is not broken
        assert bool((r[c][order][1:][same] == r[c][order][:-1][same]).all())


def test_permuting_the_pixels_permutes_the_matched_map():
    f, s = maps(seed=2)
    table = hr.quantile_table(s, 64)
    C, H, W = f.shape
    perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))
    r = hr.matched(f, table, 256).reshape(C, -1)
    rp = hr.matched(f.reshape(C, -1)[:, perm].reshape(C, H, W), table, 256).reshape(C, -1)
    assert torch.equal(rp, r[:, perm])
    for a, b in zip(hr.state(f, 256), hr.state(f.reshape(C, -1)[:, perm].reshape(C, H, W), 256)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("bins,knots", PARAMS)
def test_a_constant_and_an_all_zero_channel_match_the_lowest_quantile(bins, knots):
    f, s = maps(seed=4)
    f[1] = 0.75
    f[3] = 0.0
    table = hr.quantile_table(s, knots)
    lo, hi, cum = hr.state(f, bins)
    N = f.shape[1] * f.shape[2]
    for c, v in ((1, 0.75), (3, 0.0)):
        assert lo[c] == hi[c] == np.float32(v)
        assert cum[c, 0] == 0 and bool((cum[c, 1:] == N).all())  # everything in bin 0
        assert bool((hr.matched(f, table, bins)[c] == table[c, 0]).all())
    assert np.isfinite(float(hr.term(f, table, bins)))
    assert bool((cum[:, -1] == N).all()) and bool((np.diff(cum, axis=1) >= 0).all())


@pytest.mark.parametrize("bins", [16, 256, 1024])
def test_the_maximum_lands_in_the_last_bin(bins):
    f, s = maps(seed=5)
    lo, hi, b, frac = hr.decide(f, bins)
    flat = f.reshape(f.shape[0], -1).float().numpy()
    for c in range(f.shape[0]):
        top = flat[c] == hi[c]
        assert top.any() and bool((b[c][top] == bins - 1).all()), c
        assert bool((frac[c] <= 1.0).all()) and bool((frac[c] >= 0.0).all())
        assert bool((b[c][flat[c] == lo[c]] == 0).all()) and bool((frac[c][flat[c] == lo[c]] == 0.0).all())
    assert b.min() >= 0 and b.max() == bins - 1
    table = hr.quantile_table(s, 64)
    r = hr.matched(f, table, bins).reshape(f.shape[0], -1)
    for c in range(f.shape[0]):  # q = 1 there: the highest knot
        assert bool((r[c][torch.from_numpy(flat[c] == hi[c])] == table[c, -1]).all())


def test_analytic_gradient_equals_autograd_with_the_matched_map_detached():
    f, s = maps(seed=6)
    table = hr.quantile_table(s, 64)
    x = f.clone().requires_grad_(True)
    hr.term(x, table, 256).backward()
    assert rel_l2(hr.backward(f, table, 256), x.grad) <= 1e-14
    r = hr.matched(f, table, 256)
    assert rel_l2(hr.backward(f, table, 256, coef=0.5, upstream=-3.0), -1.5 * (f - r)) <= 1e-15
    assert abs(float(hr.term(f, table, 256)) - float(((f - r) ** 2).mean())) <= 1e-15


def test_quantile_table_reads_the_sorted_activation_at_the_knot_centres():
    s = maps(seed=7)[1]
    C, n = s.shape[0], s.shape[1] * s.shape[2]
    srt = torch.sort(s.reshape(C, -1), dim=1).values
    for knots in (2, 64, 1024):  # fewer and more knots than pixels
        t = hr.quantile_table(s, knots)
        assert t.shape == (C, knots)
        for k in (0, 1, knots // 2, knots - 1):
            assert torch.equal(t[:, k], srt[:, min(n - 1, int(np.floor((k + 0.5) * n / knots)))])


@pytest.mark.parametrize("over", [dict(), dict(use_covariance=True), dict(normalize_gradients=False, video_style_factor=0.0)],
                         ids=["default", "covariance", "plain"])
def test_factor_zero_is_the_oracles_evaluation(over):
    from oracle.style_oracle import OracleNet, build_spec
    cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", hist_loss_factor=0.0, **over)
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    onet = OracleNet(build_spec(cfg), sd, torch.float64)
    onet.capture_content(content)
    onet.capture_style([style], cfg.style_blend_weights)
    total_o, losses_o, grad_o = onet.feval(init)
    net = hr.build(content, [style], cfg, sd)
    assert net.hist_targets == {}
    total, losses, grad = net.feval(init)
    assert sorted(losses) == sorted(losses_o)
    for i in losses:
        assert abs(float(losses[i]) - float(losses_o[i])) <= 1e-12 * abs(float(losses_o[i]))
    assert abs(float(total) - float(total_o)) <= 1e-12 * abs(float(total_o))
    assert rel_l2(grad, grad_o) <= 1e-12


def test_a_factor_raises_the_loss_of_every_style_layer_and_of_nothing_else():
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    vals = {}
    for on in (False, True):
        cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", video_style_factor=0.0, normalize_gradients=False,
                       **(dict(hist_loss_factor=0.5, hist_loss_bins=64, hist_loss_knots=128) if on else {}))
        net = hr.build(content, [style], cfg, sd)
        vals[on] = (net, net.feval(init)[1])
    net = vals[True][0]
    style_slots = [i for i, l in enumerate(net.spec) if l.kind == "style"]
    assert len(style_slots) == 3 and sorted(net.hist_targets) == style_slots
    h = net.hist_terms(init)
    for i in style_slots:
        assert net.hist_targets[i].shape[1] == 128
        assert float(vals[True][1][i]) > float(vals[False][1][i]), i
        grown = float(vals[True][1][i]) - float(vals[False][1][i])  # factor x h x strength, nothing else
        assert abs(grown - 0.5 * h[i] * net.strength[i]) <= 1e-9 * grown, i
    for i in vals[False][1]:
        if i not in style_slots:
            assert float(vals[True][1][i]) == float(vals[False][1][i])


def test_two_styles_blend_their_tables():
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    other = torch.rand(1, 3, 30, 20, generator=torch.Generator().manual_seed(8)).double() * 255 - 120
    kw = dict(style_layers="relu1_1,relu2_1", content_layers="relu2_2", hist_loss_factor=1.0, hist_loss_knots=64)
    both = hr.build(content, [style, other], make_cfg(style_blend_weights=[0.25, 0.75], **kw), sd)
    one = hr.build(content, [style], make_cfg(style_blend_weights=[1.0], **kw), sd)
    two = hr.build(content, [other], make_cfg(style_blend_weights=[1.0], **kw), sd)
    for i in both.hist_targets:
        assert torch.equal(both.hist_targets[i], 0.25 * one.hist_targets[i] + 0.75 * two.hist_targets[i])
        assert bool((both.hist_targets[i][:, 1:] >= both.hist_targets[i][:, :-1]).all())  # a blend of quantile functions is one


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_feat_hist_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if n.startswith("maua_feat_hist_")) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("feat_hist_supported", "feat_hist_workspace_bytes", "feat_hist_state_bytes", "feat_hist_fwd",
                                                   "feat_hist_bwd", "feat_hist_quantiles"))
    assert hip.lib().maua_abi_version() == 2


def test_refused_arguments_answer_zero_without_a_gpu(libpath):
    import hip
    L = hip.lib()
    for ok in ((64, 1024, 1024, 256, 1024), (1, 1, 1, 16, 2), (65536, 1, (1 << 30) - 1, 1024, 4096), (512, 64, 64, 256, 1024)):
        assert L.maua_feat_hist_supported(*ok) == 1 and L.maua_feat_hist_workspace_bytes(*ok) > 0, ok
    for bad in ((0, 8, 8, 256, 1024), (65537, 8, 8, 256, 1024), (-1, 8, 8, 256, 1024), (3, 0, 8, 256, 1024), (3, 8, 0, 256, 1024),
                (3, -8, 8, 256, 1024), (3, -8, -8, 256, 1024), (3, 1 << 15, 1 << 15, 256, 1024), (3, 2147483647, 2147483647, 256, 1024),
                (3, 8, 8, 15, 1024), (3, 8, 8, 1025, 1024), (3, 8, 8, 0, 1024), (3, 8, 8, -256, 1024), (3, 8, 8, 256, 1), (3, 8, 8, 256, 4097),
                (3, 8, 8, 256, 0), (3, 8, 8, 256, -2)):
        assert L.maua_feat_hist_supported(*bad) == 0, bad
        assert L.maua_feat_hist_workspace_bytes(*bad) == 0, bad
    for c, bins in ((0, 256), (65537, 256), (3, 15), (3, 1025), (-3, 256)):
        assert L.maua_feat_hist_state_bytes(c, bins) == 0, (c, bins)


def test_state_and_workspace_sizes_follow_the_documented_layout(libpath):
    """State: per channel lo, hi and cum[0 .. bins], four bytes each.  Workspace: per (channel, chunk) one fp64 partial sum and one fp32
    (min, max) pair, the chunks those of the launch plan - a function of (C, H W) alone."""
    import hip
    L = hip.lib()
    for c in (1, 3, 64, 512, 65536):
        for bins in (16, 256, 1024):
            assert L.maua_feat_hist_state_bytes(c, bins) == c * (bins + 3) * 4
    assert plan(64, 1 << 20) == (32, 32768) and plan(512, 4096) == (4, 1024)   # both fill the chip: 2048 workgroups
    assert plan(2, 257 * 259) == (66, 1024) and 257 * 259 - 65 * 1024 == 3     # the split shape of tests/test_feat_hist_gpu.py
    assert plan(3, 35) == (1, 1024) and plan(4096, 1 << 20) == (1, 1 << 20)
    for c, h, w in ((64, 1024, 1024), (512, 64, 64), (2, 257, 259), (3, 5, 7), (70, 9, 33), (130, 20, 35), (4096, 1024, 1024), (1, 1, (1 << 30) - 1)):
        want = c * plan(c, h * w)[0] * 16
        for bins, knots in PARAMS:
            assert L.maua_feat_hist_workspace_bytes(c, h, w, bins, knots) == want, (c, h, w, bins, knots)
        assert hip.feat_hist_workspace_bytes(c, h, w, 256, 1024) == want and hip.feat_hist_state_bytes(c, 256) == c * 259 * 4
        assert hip.feat_hist_supported(c, h, w, 256, 1024)


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: MAUA_E_INVAL (-1).  Channels, planes, bins or knots outside their bounds: MAUA_E_UNSUPPORTED (-2).  A workspace one
    byte short: MAUA_E_WORKSPACE (-3).  All before any launch - the pointers handed over here are host memory no kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_double * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    big = 1 << 30
    assert L.maua_feat_hist_fwd(None, None, None, None, 3, 5, 7, 256, 64, None, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_feat_hist_bwd(None, None, None, None, 1.0, None, 3, 5, 7, 256, 64, 0, None) == -1
    assert b"null" in L.maua_last_error()
    for hole in range(5):  # f, table, state, loss, workspace
        a = [ptr] * 5
        a[hole] = None
        assert L.maua_feat_hist_fwd(a[0], a[1], a[2], a[3], 3, 5, 7, 256, 64, a[4], big, None) == -1, hole
    for hole in (0, 1, 2, 4):  # f, table, state, gx; a null upstream is allowed and the shape check comes next
        a = [ptr] * 5
        a[hole] = None
        assert L.maua_feat_hist_bwd(a[0], a[1], a[2], a[3], 1.0, a[4], 3, 5, 7, 256, 64, 0, None) == -1, hole
    for c, h, w, bins, knots in ((0, 5, 7, 256, 64), (65537, 5, 7, 256, 64), (3, 0, 7, 256, 64), (3, 5, 0, 256, 64), (3, 1 << 15, 1 << 15, 256, 64),
                                 (3, 1, 1 << 30, 256, 64), (3, 5, 7, 15, 64), (3, 5, 7, 1025, 64), (3, 5, 7, 256, 1), (3, 5, 7, 256, 4097)):
        assert L.maua_feat_hist_fwd(ptr, ptr, ptr, ptr, c, h, w, bins, knots, ptr, big, None) == -2, (c, h, w, bins, knots)
        assert b"bins" in L.maua_last_error()
        assert L.maua_feat_hist_bwd(ptr, ptr, ptr, None, 1.0, ptr, c, h, w, bins, knots, 0, None) == -2, (c, h, w, bins, knots)
        assert L.maua_feat_hist_bwd(ptr, ptr, ptr, ptr, 1.0, ptr, c, h, w, bins, knots, 1, None) == -2, (c, h, w, bins, knots)
    need = L.maua_feat_hist_workspace_bytes(2, 257, 259, 256, 64)
    assert need == 2 * 66 * 16
    assert L.maua_feat_hist_fwd(ptr, ptr, ptr, ptr, 2, 257, 259, 256, 64, ptr, need - 1, None) == -3  # one byte short
    assert b"workspace" in L.maua_last_error()
    assert L.maua_feat_hist_fwd(ptr, ptr, ptr, ptr, 2, 257, 259, 256, 64, ptr, 0, None) == -3


def test_a_guided_module_with_a_histogram_factor_raises():
    import loss
    m = loss.StyleLoss(1.0)
    m.hist_loss_factor = 0.5
    m._guide = torch.ones(1, 8, 8)
    m.mode = "loss"
    with pytest.raises(NotImplementedError, match="guides and hist_loss_factor"):
        m(torch.zeros(1, 3, 8, 8))
    m.mode = "capture"
    with pytest.raises(NotImplementedError, match="guides and hist_loss_factor"):
        m(torch.zeros(1, 3, 8, 8))


def test_the_attributes_are_no_constructor_arguments_and_reset_clears_the_target():
    import inspect
    import loss
    m = loss.StyleLoss(1.0)
    assert (m.hist_loss_factor, m.hist_loss_bins, m.hist_loss_knots) == (0.0, 256, 1024) and m.hist_target is None
    assert not any(p.startswith("hist_") for p in inspect.signature(loss.StyleLoss.__init__).parameters)
    m.hist_target = torch.zeros(3, 1024)
    m.reset_targets()
    assert m.hist_target is None
    with pytest.raises(ValueError, match="one frame"):
        loss._FeatHistFn.apply(torch.zeros(2, 3, 8, 8), torch.zeros(3, 64), 256)


def test_engine_and_optim_divert_a_histogram_module_whatever_terms_engine_says():
    import engine
    import loss
    import optim
    for terms_engine in (False, True):
        m = loss.StyleLoss(1.0)
        m.hist_loss_factor, m.terms_engine = 0.5, terms_engine
        assert optim._histogrammed([m]) and not optim._shifted([m]) and not optim._mirrored([m]) and not optim._histogrammed([loss.StyleLoss(1.0)])
        assert optim._terms_on_module_path([m]) == "feature-histogram StyleLoss runs on the module path"
        with pytest.raises(engine.UnsupportedNet, match="feature-histogram StyleLoss runs on the module path"):
            engine.StyleEngine(torch.nn.Sequential(m), [m])
        net = torch.nn.Sequential(m)
        net.style_losses = [m]
        assert optim._engine_of(net) is None and not getattr(net, "_maua_engine_refused", False)
        x = torch.zeros(2, 3, 8, 8)
        with pytest.raises(engine.UnsupportedNet, match="frame batches"):
            optim.optimize_frames(x, [x[:1]], x, 1, None, net, [m])
        m.target = torch.zeros(3, 3)
        assert optim._style_targets_missing(net)  # (the Gram target alone does not do: the factor was switched on after a capture)
        m.hist_target = torch.zeros(3, 1024)
        assert not optim._style_targets_missing(net)
    assert optim._terms_on_module_path([loss.StyleLoss(1.0)]) is None


def test_preset_keys_reach_the_modules(tmp_path):
    """The three keys are no flags (the flag surface is the reference's): they arrive through --load_args, as flip_factor does."""
    import config
    preset = tmp_path / "hist.json"
    preset.write_text(json.dumps({"hist_loss_factor": 1.5, "hist_loss_bins": 64, "hist_loss_knots": 128}))
    args = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(preset)])
    assert (args.hist_loss_factor, args.hist_loss_bins, args.hist_loss_knots) == (1.5, 64, 128)
    assert not any(flag.startswith("hist_loss") for flag, _ in config._FLAGS)
    only = tmp_path / "only.json"
    only.write_text(json.dumps({"hist_loss_factor": 1.0}))
    factor = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(only)])
    plain = config.get_args(["--content", "c.png", "--style", "s.png"])
    assert not hasattr(plain, "hist_loss_factor")

    import models
    for a, want in ((args, (1.5, 64, 128)), (factor, (1.0, 256, 1024)), (plain, (0.0, 256, 1024))):
        cnn = models.VGG(models.build_sequential(models.channel_list["VGG-19"], a.pooling))
        net, _ = models.assemble(cnn.features, models.vgg19_dict, a)
        assert len(net.style_losses) == 5
        assert all((m.hist_loss_factor, m.hist_loss_bins, m.hist_loss_knots) == want for m in net.style_losses)
        assert all(m.hist_target is None for m in net.style_losses)
