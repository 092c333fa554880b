"""Sliced Wasserstein style loss without a GPU: the directions (unit rows, the same bits from loss.swd_directions and the restatement, other
bits for another seed, index or count), the restatement with the identity as its directions against the feature-histogram restatement, its
analytic gradient against autograd, factor 0 against HistNet, the binding table, the queries and the documented sizes, the host-side argument
checks of the entry points, the preset keys on their way into the modules and the three refusals."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

import feat_hist_restatement as hr
import swd_restatement as wr
import synth
from conftest import REPO, make_cfg, rel_l2

NAMES = ["maua_swd_bwd", "maua_swd_match", "maua_swd_project", "maua_swd_state_bytes", "maua_swd_supported", "maua_swd_workspace_bytes"]
PARAMS = [(16, 2), (256, 1024), (1024, 64)]


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


def maps(C=5, H=9, W=13, seed=1, hs=11, ws=17):
    gen = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(C, H, W, generator=gen) + 0.3)
    s = torch.relu(2 * torch.randn(C, hs, ws, generator=gen) + 1)
    return f.double(), s.double()


def fh_plan(c, n):
    """csrc/feat_hist.hpp fh_plan: chunks of a row."""
    grains = -(-n // 1024)
    want = max(1, min(-(-2048 // c), grains))
    chunk = -(-(-(-n // want)) // 1024) * 1024
    return -(-n // chunk)


def tile_blocks(m, n):
    """csrc/swd.hip sw_ta: 32-row blocks of a workgroup's tile - by the rows alone (1 up to 32, 2 up to 64, else 4) for a product of fewer than
    64 workgroups of 32 rows; else the largest of these that still gives 512 workgroups, 1 if none does."""
    nt = -(-n // 256)
    by_rows = 1 if m <= 32 else 2 if m <= 64 else 4
    if -(-m // 32) * nt < 64:
        return by_rows
    ta = by_rows
    while ta > 1:
        if -(-m // (32 * ta)) * nt >= 512:
            return ta
        ta //= 2
    return 1


def slabs(d, n):
    """csrc/swd.hip sw_plan: workgroups of the projection along the pixels - spans of tiles of 256 pixels, about 1024 workgroups over the row
    tiles."""
    nt = -(-n // 256)
    span = -(-nt // max(1, 1024 // -(-d // (32 * tile_blocks(d, n)))))
    return -(-nt // span)


def test_directions_are_unit_rows_and_a_function_of_seed_index_and_shape():
    import loss
    for c, d, seed, index in ((3, 5, 0, 0), (64, 64, 0, 0), (128, 16, 3, 1), (256, 256, 7, 2)):
        v = loss.swd_directions(c, d, seed, index)
        assert v.shape == (d, c) and v.dtype == torch.float32 and not v.is_cuda
        assert float((v.double().norm(dim=1) - 1).abs().max()) <= 1e-7
        assert torch.equal(v, wr.directions(c, d, seed, index))
        assert torch.equal(v, loss.swd_directions(c, d, seed, index))
    base = loss.swd_directions(64, 64, 0, 0)
    assert not torch.equal(base, loss.swd_directions(64, 64, 1, 0))
    assert not torch.equal(base, loss.swd_directions(64, 64, 0, 1))
    assert not torch.equal(base, loss.swd_directions(64, 16, 0, 0)) and not torch.equal(base[:, :32], loss.swd_directions(32, 64, 0, 0))
    assert torch.equal(loss.swd_directions(64, 64, 1, 0), wr.directions(64, 64, 0, 8191))  # the seed of the generator is seed * 8191 + index


@pytest.mark.parametrize("bins,knots", PARAMS)
def test_identity_directions_give_the_feature_histogram_term_and_gradient(bins, knots):
    f, s = maps()
    eye = torch.eye(f.shape[0])
    tab = wr.table(s, eye, knots)
    assert torch.equal(tab, hr.quantile_table(s, knots))
    assert float(wr.term(f, eye, tab, bins)) == float(hr.term(f, tab, bins))
    assert torch.equal(wr.backward(wr.project(f, eye), eye, tab, bins), hr.backward(f, tab, bins))


@pytest.mark.parametrize("d", [3, 5, 8])
def test_analytic_gradient_equals_autograd_with_the_matched_map_detached(d):
    f, s = maps(seed=6)
    v = wr.directions(f.shape[0], d, 2, 1)
    tab = wr.table(s, v, 64)
    x = f.clone().requires_grad_(True)
    wr.term(x, v, tab, 256).backward()
    p = wr.project(f, v)
    assert rel_l2(wr.backward(p, v, tab, 256), x.grad) <= 1e-13
    g = wr.residual(p, tab, 256)
    assert abs(float(wr.term(f, v, tab, 256)) - float((g ** 2).mean())) <= 1e-15
    want = -1.5 * (v.double().t() @ g.reshape(d, -1)).reshape(f.shape)
    assert rel_l2(wr.backward(p, v, tab, 256, coef=0.5, upstream=-3.0), want) <= 1e-15


def test_factor_zero_is_the_histogram_networks_evaluation_and_a_factor_raises_the_style_layers_alone():
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    kw = dict(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", video_style_factor=0.0, normalize_gradients=False)
    plain = hr.build(content, [style], make_cfg(**kw), sd).feval(init)
    off = wr.build(content, [style], make_cfg(swd_factor=0.0, **kw), sd)
    assert off.swd_targets == {}
    got = off.feval(init)
    assert float(got[0]) == float(plain[0]) and torch.equal(got[2], plain[2])
    on = wr.build(content, [style], make_cfg(swd_factor=0.5, swd_directions=16, swd_bins=64, swd_knots=128, swd_seed=3, **kw), sd)
    slots = on.style_slots()
    assert len(slots) == 3 and sorted(on.swd_targets) == slots
    acts, _ = on.net._forward(init)
    losses = on.feval(init)[1]
    for index, i in enumerate(slots):
        C = acts[i].shape[1]
        assert on.swd_targets[i].shape == (16, 128) and torch.equal(on.swd_dirs[i], wr.directions(C, 16, 3, index))
        s = float(wr.term(acts[i][0].detach(), on.swd_dirs[i], on.swd_targets[i], 64))
        grown = float(losses[i]) - float(plain[1][i])
        assert s > 0 and abs(grown - 0.5 * s * on.strength[i]) <= 1e-9 * grown, i
    for i in plain[1]:
        if i not in slots:
            assert float(losses[i]) == float(plain[1][i])


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_swd_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if n.startswith("maua_swd_")) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("swd_supported", "swd_workspace_bytes", "swd_state_bytes", "swd_project", "swd_match", "swd_bwd"))
    assert hip.lib().maua_abi_version() == 2


def test_the_queries_answer_without_a_gpu_and_sizes_follow_the_documented_layout(libpath):
    """State: the feature-histogram record for D directions, D (bins + 3) words.  Workspace: per (direction, chunk of the matcher's plan) one
    fp64 partial sum, then per (direction, workgroup of the projection along the pixels) one fp32 (min, max) pair."""
    import hip
    L = hip.lib()
    for ok in ((64, 64, 1024, 1024, 256, 1024), (1, 1, 1, 1, 16, 2), (4096, 4096, 1, (1 << 30) - 1, 1024, 4096), (512, 16, 64, 64, 256, 1024)):
        assert L.maua_swd_supported(*ok) == 1 and L.maua_swd_workspace_bytes(*ok) > 0, ok
    for bad in ((0, 8, 8, 8, 256, 1024), (4097, 8, 8, 8, 256, 1024), (-1, 8, 8, 8, 256, 1024), (8, 0, 8, 8, 256, 1024), (8, 4097, 8, 8, 256, 1024),
                (8, -8, 8, 8, 256, 1024), (3, 3, 0, 8, 256, 1024), (3, 3, 8, 0, 256, 1024), (3, 3, -8, -8, 256, 1024), (3, 3, 1 << 15, 1 << 15, 256, 1024),
                (3, 3, 2147483647, 2147483647, 256, 1024), (3, 3, 8, 8, 15, 1024), (3, 3, 8, 8, 1025, 1024), (3, 3, 8, 8, 0, 1024),
                (3, 3, 8, 8, 256, 1), (3, 3, 8, 8, 256, 4097), (3, 3, 8, 8, 256, -2)):
        assert L.maua_swd_supported(*bad) == 0, bad
        assert L.maua_swd_workspace_bytes(*bad) == 0, bad
    for d in (1, 3, 64, 512, 4096):
        for bins in (16, 256, 1024):
            assert L.maua_swd_state_bytes(d, bins) == d * (bins + 3) * 4 == L.maua_feat_hist_state_bytes(d, bins)
    for d, bins in ((0, 256), (4097, 256), (3, 15), (3, 1025), (-3, 256)):
        assert L.maua_swd_state_bytes(d, bins) == 0, (d, bins)
    assert [tile_blocks(c, (1024 // k) ** 2) for c, k in ((64, 1), (128, 2), (256, 4), (512, 8), (512, 16))] == [2, 4, 4, 2, 1]  # a 1024 x 1024 job
    assert [tile_blocks(m, n) for m, n in ((5, 35), (3, 35), (70, 297), (64, 700), (130, 700), (96, 256), (2, 257 * 259))] == [1, 1, 4, 2, 4, 4, 1]
    assert slabs(64, 1 << 20) == 1024 and slabs(512, 1 << 14) == 64 and slabs(2, 257 * 259) == 261 and slabs(5, 35) == 1
    for c, d, h, w in ((64, 64, 1024, 1024), (512, 512, 128, 128), (2, 2, 257, 259), (3, 5, 5, 7), (70, 70, 9, 33), (130, 64, 20, 35),
                       (64, 96, 16, 16), (512, 16, 64, 64)):
        want = d * fh_plan(d, h * w) * 8 + d * slabs(d, h * w) * 8
        for bins, knots in PARAMS:
            assert L.maua_swd_workspace_bytes(c, d, h, w, bins, knots) == want, (c, d, h, w, bins, knots)
        assert hip.swd_workspace_bytes(c, d, h, w, 256, 1024) == want and hip.swd_state_bytes(d, 256) == d * 259 * 4
        assert hip.swd_supported(c, d, h, w, 256, 1024)


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: MAUA_E_INVAL (-1).  Shapes outside their bounds: MAUA_E_UNSUPPORTED (-2).  A workspace one byte short:
    MAUA_E_WORKSPACE (-3).  All before any launch - the pointers handed over here are host memory no kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_double * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    big = 1 << 30
    assert L.maua_swd_project(None, None, None, None, 3, 5, 5, 7, 256, None, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_swd_match(None, None, None, None, 5, 5, 7, 256, 64, None, 0, None) == -1
    assert L.maua_swd_bwd(None, None, None, 1.0, None, 3, 5, 5, 7, 0, None) == -1
    for hole in range(3):  # f, dirs, proj
        a = [ptr] * 3
        a[hole] = None
        assert L.maua_swd_project(a[0], a[1], a[2], ptr, 3, 5, 5, 7, 256, ptr, big, None) == -1, hole
        assert L.maua_swd_project(a[0], a[1], a[2], None, 3, 5, 5, 7, 256, None, 0, None) == -1, hole
    assert L.maua_swd_project(ptr, ptr, ptr, ptr, 3, 5, 5, 7, 256, None, 0, None) == -1  # a state needs its workspace
    for hole in range(5):  # proj, table, state, loss, workspace
        a = [ptr] * 5
        a[hole] = None
        assert L.maua_swd_match(a[0], a[1], a[2], a[3], 5, 5, 7, 256, 64, a[4], big, None) == -1, hole
    for hole in (0, 1, 3):  # g, dirs_t, gx; a null upstream is allowed and the shape check comes next
        a = [ptr] * 4
        a[hole] = None
        assert L.maua_swd_bwd(a[0], a[1], a[2], 1.0, a[3], 3, 5, 5, 7, 0, None) == -1, hole
    for c, d, h, w in ((0, 5, 5, 7), (4097, 5, 5, 7), (3, 0, 5, 7), (3, 4097, 5, 7), (3, 5, 0, 7), (3, 5, 5, 0), (3, 5, 1 << 15, 1 << 15), (3, 5, 1, 1 << 30)):
        assert L.maua_swd_project(ptr, ptr, ptr, ptr, c, d, h, w, 256, ptr, big, None) == -2, (c, d, h, w)
        assert L.maua_swd_project(ptr, ptr, ptr, None, c, d, h, w, 256, None, 0, None) == -2, (c, d, h, w)
        assert b"directions" in L.maua_last_error()
        assert L.maua_swd_bwd(ptr, ptr, None, 1.0, ptr, c, d, h, w, 0, None) == -2, (c, d, h, w)
        assert L.maua_swd_bwd(ptr, ptr, ptr, 1.0, ptr, c, d, h, w, 1, None) == -2, (c, d, h, w)
    for d, h, w, bins, knots in ((0, 5, 7, 256, 64), (4097, 5, 7, 256, 64), (5, 0, 7, 256, 64), (5, 1, 1 << 30, 256, 64), (5, 5, 7, 15, 64),
                                 (5, 5, 7, 1025, 64), (5, 5, 7, 256, 1), (5, 5, 7, 256, 4097)):
        assert L.maua_swd_match(ptr, ptr, ptr, ptr, d, h, w, bins, knots, ptr, big, None) == -2, (d, h, w, bins, knots)
        assert b"bins" in L.maua_last_error()
    for bins in (15, 1025, 0):
        assert L.maua_swd_project(ptr, ptr, ptr, ptr, 3, 5, 5, 7, bins, ptr, big, None) == -2, bins
    need = L.maua_swd_workspace_bytes(2, 2, 257, 259, 256, 64)
    assert need == 2 * 66 * 8 + 2 * 261 * 8
    assert L.maua_swd_project(ptr, ptr, ptr, ptr, 2, 2, 257, 259, 256, ptr, need - 1, None) == -3  # one byte short
    assert b"workspace" in L.maua_last_error()
    assert L.maua_swd_match(ptr, ptr, ptr, ptr, 2, 257, 259, 256, 64, ptr, need - 1, None) == -3
    assert L.maua_swd_match(ptr, ptr, ptr, ptr, 2, 257, 259, 256, 64, ptr, 0, None) == -3


def test_preset_keys_reach_the_modules_with_their_defaults(tmp_path):
    """The five keys are no flags (the flag surface is the reference's): they arrive through --load_args, as hist_loss_factor does."""
    import config
    import models
    preset = tmp_path / "swd.json"
    preset.write_text(json.dumps({"swd_factor": 1.5, "swd_directions": 16, "swd_seed": 3, "swd_bins": 64, "swd_knots": 128}))
    args = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(preset)])
    assert (args.swd_factor, args.swd_directions, args.swd_seed, args.swd_bins, args.swd_knots) == (1.5, 16, 3, 64, 128)
    assert not any(flag.startswith("swd") for flag, _ in config._FLAGS)
    only = tmp_path / "only.json"
    only.write_text(json.dumps({"swd_factor": 1.0}))
    factor = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(only)])
    plain = config.get_args(["--content", "c.png", "--style", "s.png"])
    assert not hasattr(plain, "swd_factor")
    for a, want in ((args, (1.5, 16, 3, 64, 128)), (factor, (1.0, 0, 0, 256, 1024)), (plain, (0.0, 0, 0, 256, 1024))):
        cnn = models.VGG(models.build_sequential(models.channel_list["VGG-19"], a.pooling))
        net, _ = models.assemble(cnn.features, models.vgg19_dict, a)
        assert len(net.style_losses) == 5
        assert all((m.swd_factor, m.swd_directions, m.swd_seed, m.swd_bins, m.swd_knots) == want for m in net.style_losses)
        assert [m.swd_index for m in net.style_losses] == [0, 1, 2, 3, 4]
        assert all(m.swd_target is None and m._swd_dirs is None for m in net.style_losses)


def test_the_attributes_are_no_constructor_arguments_and_reset_clears_target_and_directions():
    import inspect
    import loss
    m = loss.StyleLoss(1.0)
    assert (m.swd_factor, m.swd_directions, m.swd_seed, m.swd_bins, m.swd_knots, m.swd_index) == (0.0, 0, 0, 256, 1024, 0)
    assert m.swd_target is None and m._swd_dirs is None
    assert not any(p.startswith("swd_") for p in inspect.signature(loss.StyleLoss.__init__).parameters)
    m.swd_target = torch.zeros(3, 1024)
    m._swd_dirs = (torch.eye(3), torch.eye(3))
    m.reset_targets()
    assert m.swd_target is None and m._swd_dirs is None
    with pytest.raises(ValueError, match="one frame"):
        loss._SwdFn.apply(torch.zeros(2, 3, 8, 8), torch.eye(3), torch.eye(3), torch.zeros(3, 64), 256)


def test_a_guided_module_with_a_sliced_factor_raises():
    import loss
    m = loss.StyleLoss(1.0)
    m.swd_factor = 0.5
    m._guide = torch.ones(1, 8, 8)
    for mode in ("loss", "capture"):
        m.mode = mode
        with pytest.raises(NotImplementedError, match="guides and swd_factor > 0 together are not implemented"):
            m(torch.zeros(1, 3, 8, 8))


def test_a_target_that_was_not_captured_or_has_another_shape_raises():
    import loss
    m = loss.StyleLoss(1.0)
    m.name = "style 3"
    m.swd_factor = 1.0
    frame = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="style 3: sliced Wasserstein target not captured"):
        m._swd_terms(frame, 0.0)
    m.swd_target = torch.zeros(5, 1024)
    with pytest.raises(RuntimeError, match=r"sliced Wasserstein target of shape \(5, 1024\) for 3 directions and 1024 knots: capture again"):
        m._swd_terms(frame, 0.0)
    m.swd_directions, m.swd_knots = 5, 64
    with pytest.raises(RuntimeError, match="capture again"):
        m._swd_terms(frame, 0.0)


def test_engine_and_optim_divert_a_sliced_module_whatever_terms_engine_says():
    import engine
    import loss
    import optim
    reason = "sliced-Wasserstein StyleLoss runs on the module path"
    for terms_engine in (False, True):
        m = loss.StyleLoss(1.0)
        m.swd_factor, m.terms_engine = 0.5, terms_engine
        assert optim._sliced([m]) and not optim._histogrammed([m]) and not optim._patch_matched([m]) and not optim._sliced([loss.StyleLoss(1.0)])
        assert optim._terms_on_module_path([m]) == reason
        with pytest.raises(engine.UnsupportedNet, match=reason):
            engine.StyleEngine(torch.nn.Sequential(m), [m])
        net = torch.nn.Sequential(m)
        net.style_losses = [m]
        assert optim._engine_of(net) is None and not getattr(net, "_maua_engine_refused", False)
        m.target = torch.zeros(3, 3)
        assert optim._style_targets_missing(net)  # (the Gram target alone does not do: the factor was switched on after a capture)
        m.swd_target = torch.zeros(3, 1024)
        assert not optim._style_targets_missing(net)
    assert optim._terms_on_module_path([loss.StyleLoss(1.0)]) is None
