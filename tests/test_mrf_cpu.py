"""MRF patch-matching style loss without a GPU: the restatement (tests/mrf_restatement.py) - its gather gradient against autograd of the
unfolded form, the lowest index among equal scores, the planted answer -, the bank's stride rule, cap and stacking (loss.mrf_grid against
the restatement's), the binding table, the host-side argument checks of the entry points, the documented sizes of state and workspace, the
refusals of the modules and the preset keys on their way into the modules."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

import mrf_restatement as mr
from conftest import REPO, rel_l2

NAMES = ["maua_mrf_bank", "maua_mrf_bwd", "maua_mrf_fwd", "maua_mrf_state_bytes", "maua_mrf_supported", "maua_mrf_workspace_bytes"]


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


def maps(C=5, H=9, W=13, seed=1, hs=11, ws=17):
    gen = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(C, H, W, generator=gen) + 0.3), torch.relu(torch.randn(C, hs, ws, generator=gen) + 0.3)


def plan(q, p):
    """csrc/mrf.hip mrf_plan: (slices, tiles per slice) - about 4096 workgroups of 256 queries, at most 64 slices, tiles of 128 patches."""
    qtiles, tiles = -(-q // 256), -(-p // 128)
    want = max(1, min(-(-4096 // qtiles), 64, tiles))
    per = -(-tiles // want)
    return -(-tiles // per), per


def gather_plan(c, hw):
    """mrf_gather_plan: (pixel blocks, channel chunks) - about 2048 workgroups of 256 pixels."""
    pb = -(-hw // 256)
    want = max(1, min(-(-2048 // pb), c))
    per = -(-c // want)
    return pb, -(-c // per)


def test_the_gather_gradient_is_autograd_of_the_unfolded_form():
    for seed, stride in ((1, 1), (2, 2), (3, 3)):
        f, s = maps(seed=seed)
        s_map, origin, inv, _ = mr.build_bank([s], stride, 10000)
        nn = mr.nearest(mr.scores(f, s_map, origin, inv))
        a, b = mr.gradient(f, s_map, origin, nn), mr.gather_gradient(f, s_map, origin, nn)
        assert rel_l2(b, a) <= 1e-14
        assert rel_l2(mr.gather_gradient(f, s_map, origin, nn, coef=0.37), a * (0.37 * 9 * 5 * 7 * 11 / 2.0)) <= 1e-14
        # and it is the derivative of the loss with nn held fixed: a central difference along a random direction
        d = torch.randn(f.shape, generator=torch.Generator().manual_seed(9)).double()
        eps = 1e-6
        num = (mr.loss(f.double() + eps * d, s_map, origin, nn) - mr.loss(f.double() - eps * d, s_map, origin, nn)) / (2 * eps)
        assert abs(float(num) - float((a * d).sum())) <= 1e-7 * abs(float(num))


def test_equal_scores_go_to_the_lowest_index_and_a_cut_out_window_finds_its_origin():
    sc = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 2.0, 3.0]], dtype=torch.float64)
    assert mr.nearest(sc).tolist() == [1, 0, 3]
    _, s = maps(hs=12, ws=15)
    s_map, origin, inv, _ = mr.build_bank([s], 1, 10000)
    f = s[:, 3:9, 4:12].clone()
    nn = mr.nearest(mr.scores(f, s_map, origin, inv))
    want = torch.tensor([(3 + y) * 15 + 4 + x for y in range(4) for x in range(6)])
    assert torch.equal(origin.long()[nn], want)
    assert float(mr.loss(f, s_map, origin, nn)) == 0.0 and not bool(mr.gather_gradient(f, s_map, origin, nn).any())


def test_the_stride_rule_and_the_cap():
    import loss
    for sizes, stride, cap in (([(12, 15)], 1, 10000), ([(12, 15)], 2, 10000), ([(12, 15)], 1, 129), ([(12, 15)], 1, 30), ([(12, 15)], 3, 1),
                               ([(64, 64)], 2, 16384), ([(258, 258)], 2, 16384), ([(258, 258), (130, 200)], 2, 16384), ([(3, 3)], 2, 1),
                               ([(9, 40), (20, 11), (5, 5)], 1, 200)):
        s, origins = loss.mrf_grid(sizes, stride, cap)
        s_r, origins_r = mr.grid(sizes, stride, cap)
        assert (s, origins) == (s_r, origins_r), (sizes, stride, cap)
        count = lambda st: sum(len(range(0, h - 2, st)) * len(range(0, w - 2, st)) for h, w in sizes)  # noqa: E731
        assert len(origins) == count(s) <= cap and s >= stride
        assert s == stride or count(s - 1) > cap  # the smallest such stride
        assert len(set(origins)) == len(origins) and origins == sorted(origins)
    assert loss.mrf_grid([(12, 15)], 1, 10000)[0] == 1 and len(loss.mrf_grid([(12, 15)], 1, 10000)[1]) == 130
    assert loss.mrf_grid([(12, 15)], 1, 129)[0] == 2 and loss.mrf_grid([(258, 258)], 2, 16384) == mr.grid([(258, 258)], 2, 16384)
    assert len(loss.mrf_grid([(258, 258)], 2, 16384)[1]) == 128 * 128
    assert loss.mrf_grid([(258, 258), (258, 258)], 2, 16384)[0] == 3  # 2 x 86 x 86 = 14792
    with pytest.raises(ValueError, match="at least 3 x 3"):
        loss.mrf_grid([(2, 9)], 1, 100)
    with pytest.raises(ValueError, match="mrf_max_patches"):
        loss.mrf_grid([(9, 9), (9, 9)], 1, 1)


def test_stacked_maps_of_different_widths_list_no_patch_across_two_of_them():
    import loss
    gen = torch.Generator().manual_seed(4)
    a, b = torch.rand(3, 7, 12, generator=gen) + 0.1, torch.rand(3, 9, 8, generator=gen) + 0.1
    for stride in (1, 2):
        s_map, origin, inv, s = mr.build_bank([a, b], stride, 10000)
        assert s == stride and tuple(s_map.shape) == (3, 16, 12)
        assert torch.equal(s_map[:, :7], a) and torch.equal(s_map[:, 7:, :8], b) and not bool(s_map[:, 7:, 8:].any())
        assert origin.tolist() == loss.mrf_grid([(7, 12), (9, 8)], stride, 10000)[1]  # (no patch here has norm 0)
        ys, xs = origin.long() // 12, origin.long() % 12
        in_a = (ys + 2 <= 6)
        in_b = (ys >= 7) & (ys + 2 <= 15) & (xs + 2 <= 7)
        assert bool((in_a ^ in_b).all()) and int(in_a.sum()) == len(range(0, 5, stride)) * len(range(0, 10, stride))
        got = mr.bank_patches(s_map, origin)
        own = torch.cat([mr.patches(a).reshape(5, 10, -1)[::stride, ::stride].reshape(-1, 27),
                         mr.patches(b).reshape(7, 6, -1)[::stride, ::stride].reshape(-1, 27)])
        assert torch.equal(got, own)  # every listed patch is a patch of one of the two maps
        assert torch.equal(inv, (1.0 / own.double().pow(2).sum(1).sqrt()).float())


def test_patches_of_norm_zero_are_not_listed():
    s = torch.zeros(2, 8, 9)
    s[:, 5:, 6:] = 1.0
    s_map, origin, inv, _ = mr.build_bank([s], 1, 10000)
    ys, xs = origin.long() // 9, origin.long() % 9
    assert origin.numel() == 3 * 3 and bool(((ys + 2 >= 5) & (xs + 2 >= 6)).all()) and bool(torch.isfinite(inv).all())


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_mrf_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if n.startswith("maua_mrf_")) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("mrf_supported", "mrf_workspace_bytes", "mrf_state_bytes", "mrf_bank", "mrf_fwd", "mrf_bwd"))
    assert hip.lib().maua_abi_version() == 2


def test_refused_arguments_answer_zero_and_sizes_follow_the_documented_layout(libpath):
    """State: nn[Q] and best[Q], four bytes each.  Workspace: one fp64 partial sum per workgroup of the gather pass, then per slice of
    the bank and query one fp32 score and one int32 patch - the slices a function of (Q, P) alone."""
    import hip
    L = hip.lib()
    for c, h, w, hs, ws, p in ((2, 3, 3, 3, 3, 1), (3, 5, 7, 6, 9, 28), (70, 9, 33, 12, 31, 290), (130, 20, 35, 23, 40, 209), (16, 66, 70, 67, 131, 8385),
                               (256, 256, 256, 258, 258, 16384), (1024, 3, (1 << 30) // 3, 3, 3, 1 << 20)):
        q = (h - 2) * (w - 2)
        pb, cc = gather_plan(c, h * w)
        want = pb * cc * 8 + plan(q, p)[0] * q * 8
        assert L.maua_mrf_supported(c, h, w, hs, ws, p) == 1 and L.maua_mrf_workspace_bytes(c, h, w, hs, ws, p) == want, (c, h, w, hs, ws, p)
        assert hip.mrf_workspace_bytes(c, h, w, hs, ws, p) == want and hip.mrf_state_bytes(h, w) == 8 * q and hip.mrf_supported(c, h, w, hs, ws, p)
    assert plan(1, 1) == (1, 1) and plan(35, 28) == (1, 1) and plan(217, 290) == (3, 1) and plan(594, 209) == (2, 1)
    assert plan(4352, 8385) == (33, 2)  # the last shape of tests/test_mrf_gpu.py: 66 tiles in 33 slices, so the merge has work to do
    assert plan(254 * 254, 16384) == (16, 8)
    for bad in ((0, 8, 8, 8, 8, 4), (1025, 8, 8, 8, 8, 4), (-1, 8, 8, 8, 8, 4), (3, 2, 8, 8, 8, 4), (3, 8, 2, 8, 8, 4), (3, 8, 8, 2, 8, 4),
                (3, 8, 8, 8, 2, 4), (3, -8, -8, 8, 8, 4), (3, 1 << 15, 1 << 15, 8, 8, 4), (3, 8, 8, 1 << 15, 1 << 15, 4),
                (3, 2147483647, 2147483647, 8, 8, 4), (3, 8, 8, 8, 8, 0), (3, 8, 8, 8, 8, (1 << 20) + 1), (3, 8, 8, 8, 8, -4)):
        assert L.maua_mrf_supported(*bad) == 0 and L.maua_mrf_workspace_bytes(*bad) == 0, bad
    for h, w in ((2, 8), (8, 2), (-8, -8), (1 << 15, 1 << 15), (0, 0)):
        assert L.maua_mrf_state_bytes(h, w) == 0, (h, w)


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: MAUA_E_INVAL (-1).  Channels, planes or patch counts outside their bounds: MAUA_E_UNSUPPORTED (-2).  A workspace one
    byte short: MAUA_E_WORKSPACE (-3).  All before any launch - the pointers handed over here are host memory no kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_double * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    big = 1 << 30
    shape = (3, 5, 7, 6, 9, 28)
    for hole in range(7):  # f, s, origin, inv, state, loss, workspace
        a = [ptr] * 7
        a[hole] = None
        assert L.maua_mrf_fwd(*a[:6], *shape, a[6], big, None) == -1, hole
        assert b"null" in L.maua_last_error()
    for hole in (0, 1, 2, 3, 5):  # f, s, origin, state, gx; a null upstream is allowed and the shape check comes next
        a = [ptr] * 6
        a[hole] = None
        assert L.maua_mrf_bwd(a[0], a[1], a[2], a[3], a[4], 1.0, a[5], *shape, 0, None) == -1, hole
    for hole in range(3):
        a = [ptr] * 3
        a[hole] = None
        assert L.maua_mrf_bank(*a, 3, 6, 9, 28, None) == -1, hole
    for bad in ((0, 5, 7, 6, 9, 28), (1025, 5, 7, 6, 9, 28), (3, 2, 7, 6, 9, 28), (3, 5, 2, 6, 9, 28), (3, 5, 7, 2, 9, 28), (3, 5, 7, 6, 2, 28),
                (3, 1 << 15, 1 << 15, 6, 9, 28), (3, 5, 7, 1 << 15, 1 << 15, 28), (3, 5, 7, 6, 9, 0), (3, 5, 7, 6, 9, (1 << 20) + 1)):
        assert L.maua_mrf_fwd(ptr, ptr, ptr, ptr, ptr, ptr, *bad, ptr, big, None) == -2, bad
        assert b"patches" in L.maua_last_error()
        assert L.maua_mrf_bwd(ptr, ptr, ptr, ptr, None, 1.0, ptr, *bad, 0, None) == -2, bad
        assert L.maua_mrf_bwd(ptr, ptr, ptr, ptr, ptr, 1.0, ptr, *bad, 1, None) == -2, bad
    for bad in ((0, 6, 9, 28), (1025, 6, 9, 28), (3, 2, 9, 28), (3, 6, 2, 28), (3, 1 << 15, 1 << 15, 28), (3, 6, 9, 0), (3, 6, 9, (1 << 20) + 1)):
        assert L.maua_mrf_bank(ptr, ptr, ptr, *bad, None) == -2, bad
    big_shape = (16, 66, 70, 67, 131, 8385)
    need = L.maua_mrf_workspace_bytes(*big_shape)
    assert L.maua_mrf_fwd(ptr, ptr, ptr, ptr, ptr, ptr, *big_shape, ptr, need - 1, None) == -3  # one byte short
    assert b"workspace" in L.maua_last_error()
    assert L.maua_mrf_fwd(ptr, ptr, ptr, ptr, ptr, ptr, *big_shape, ptr, 0, None) == -3


def test_a_guided_module_with_an_mrf_factor_raises():
    import loss
    m = loss.StyleLoss(1.0)
    m.mrf_factor = 0.5
    m._guide = torch.ones(1, 8, 8)
    for mode in ("loss", "capture"):
        m.mode = mode
        with pytest.raises(NotImplementedError, match="guides and mrf_factor"):
            m(torch.zeros(1, 3, 8, 8))


def test_the_attributes_are_no_constructor_arguments_and_reset_drops_the_bank():
    import inspect
    import loss
    m = loss.StyleLoss(1.0)
    assert (m.mrf_factor, m.mrf_stride, m.mrf_max_patches) == (0.0, 2, 16384) and m.mrf_bank is None and m._mrf_maps == []
    assert not any(p.startswith("mrf_") for p in inspect.signature(loss.StyleLoss.__init__).parameters)
    m.mrf_bank, m._mrf_maps = (torch.zeros(3, 5, 5), torch.zeros(1, dtype=torch.int32), torch.ones(1)), [torch.zeros(3, 5, 5)]
    m.reset_targets()
    assert m.mrf_bank is None and m._mrf_maps == []
    with pytest.raises(ValueError, match="one frame"):
        loss._MrfFn.apply(torch.zeros(2, 3, 8, 8), torch.zeros(3, 8, 8), torch.zeros(1, dtype=torch.int32), torch.ones(1))
    # a style image that takes no part in the blend gives no patches
    m.mrf_factor, m.blend_weight = 1.0, 0.0
    m._mrf_capture(torch.ones(1, 3, 5, 5))
    assert m._mrf_maps == []
    m.blend_weight = 0.25
    m._mrf_capture(torch.ones(1, 3, 5, 5))
    assert len(m._mrf_maps) == 1 and tuple(m._mrf_maps[0].shape) == (3, 5, 5)


def test_engine_and_optim_divert_an_mrf_module_whatever_terms_engine_says():
    import engine
    import loss
    import optim
    for terms_engine in (False, True):
        m = loss.StyleLoss(1.0)
        m.mrf_factor, m.terms_engine = 0.5, terms_engine
        assert optim._patch_matched([m]) and not optim._histogrammed([m]) and not optim._shifted([m]) and not optim._mirrored([m])
        assert not optim._patch_matched([loss.StyleLoss(1.0)])
        assert optim._terms_on_module_path([m]) == "MRF patch-matching StyleLoss runs on the module path"
        with pytest.raises(engine.UnsupportedNet, match="MRF patch-matching StyleLoss runs on the module path"):
            engine.StyleEngine(torch.nn.Sequential(m), [m])
        net = torch.nn.Sequential(m)
        net.style_losses = [m]
        assert optim._engine_of(net) is None and not getattr(net, "_maua_engine_refused", False)
        x = torch.zeros(2, 3, 8, 8)
        with pytest.raises(engine.UnsupportedNet, match="frame batches"):
            optim.optimize_frames(x, [x[:1]], x, 1, None, net, [m])
        m.target = torch.zeros(3, 3)
        assert optim._style_targets_missing(net)  # (the Gram target alone does not do: the factor was switched on after a capture)
        m._mrf_maps = [torch.zeros(3, 5, 5)]
        assert not optim._style_targets_missing(net)
    assert optim._terms_on_module_path([loss.StyleLoss(1.0)]) is None


def test_preset_keys_reach_the_modules(tmp_path):
    """The four keys are no flags (the flag surface is the reference's): they arrive through --load_args, as hist_loss_factor does."""
    import config
    import models
    preset = tmp_path / "mrf.json"
    preset.write_text(json.dumps({"mrf_factor": 1.5, "mrf_stride": 3, "mrf_max_patches": 4096, "mrf_layers": "relu2_1,relu5_1"}))
    args = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(preset)])
    assert (args.mrf_factor, args.mrf_stride, args.mrf_max_patches, args.mrf_layers) == (1.5, 3, 4096, "relu2_1,relu5_1")
    assert not any(flag.startswith("mrf_") for flag, _ in config._FLAGS)
    only = tmp_path / "only.json"
    only.write_text(json.dumps({"mrf_factor": 1.0}))
    factor = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(only)])
    plain = config.get_args(["--content", "c.png", "--style", "s.png"])
    assert not hasattr(plain, "mrf_factor")

    def factors(a):
        cnn = models.VGG(models.build_sequential(models.channel_list["VGG-19"], a.pooling))
        net, _ = models.assemble(cnn.features, models.vgg19_dict, a)
        assert len(net.style_losses) == 5 and all(m.mrf_bank is None for m in net.style_losses)
        return [(m.mrf_factor, m.mrf_stride, m.mrf_max_patches) for m in net.style_losses]  # relu1_1 .. relu5_1

    assert factors(args) == [(0.0, 3, 4096), (1.5, 3, 4096), (0.0, 3, 4096), (0.0, 3, 4096), (1.5, 3, 4096)]
    assert factors(factor) == [(0.0, 2, 16384), (0.0, 2, 16384), (1.0, 2, 16384), (1.0, 2, 16384), (0.0, 2, 16384)]  # the paper's layers
    assert factors(plain) == [(0.0, 2, 16384)] * 5

    wrong = tmp_path / "wrong.json"
    wrong.write_text(json.dumps({"mrf_factor": 1.0, "mrf_layers": "relu3_1,relu3_2"}))
    a = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(wrong)])
    with pytest.raises(ValueError) as e:
        factors(a)
    assert "relu3_2" in str(e.value) and "relu1_1" in str(e.value) and "relu5_1" in str(e.value)  # both lists are named
    a.mrf_factor = 0.0  # with the term off the key is not looked at
    assert factors(a) == [(0.0, 2, 16384)] * 5
    narrow = config.get_args(["--content", "c.png", "--style", "s.png", "--style_layers", "relu1_1,relu2_1", "--load_args", str(only)])
    with pytest.raises(ValueError, match="relu3_1"):
        models.assemble(models.VGG(models.build_sequential(models.channel_list["VGG-19"], narrow.pooling)).features, models.vgg19_dict, narrow)


def test_the_network_restatement_adds_the_term_to_the_named_layers_only():
    """tests/mrf_restatement.MrfNet: the named style layer's slot grows by factor x m x strength, nothing else moves, and handing the
    network its own decisions changes nothing."""
    import synth
    from conftest import make_cfg
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    vals = {}
    for on in (False, True):
        cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", video_style_factor=0.0, normalize_gradients=False,
                       **(dict(mrf_factor=0.5, mrf_stride=1, mrf_layers="relu2_1") if on else {}))
        net = mr.build_net(content, [style], cfg, sd)
        vals[on] = (net, net.feval(init))
    net = vals[True][0]
    style_slots = [i for i, l in enumerate(net.spec) if l.kind == "style"]
    assert len(style_slots) == 3 and net.mrf_slots == [style_slots[1]] and vals[False][0].mrf_slots == []
    i = net.mrf_slots[0]
    assert net.mrf_banks[i][1].numel() == 10 * 10  # the 12 x 12 map of relu2_1 at stride 1
    m = net.mrf_terms(init)[i]
    grown = float(vals[True][1][1][i]) - float(vals[False][1][1][i])
    assert m > 0 and abs(grown - 0.5 * m * net.strength[i]) <= 1e-9 * grown
    for k in vals[False][1][1]:
        if k != i:
            assert float(vals[True][1][1][k]) == float(vals[False][1][1][k])
    own = {i: net.mrf_nearest(init)[i][None, :]}
    pinned = net.feval(init, nn=own)
    assert float(pinned[0]) == float(vals[True][1][0]) and torch.equal(pinned[2], vals[True][1][2])
    assert not torch.equal(vals[True][1][2], vals[False][1][2])
