"""Mirrored-Gram style loss without a GPU: the fp64 restatement (tests/flip_restatement.py) - torch.flip against the index form, symmetry,
degenerate axes, the point mirror as LR after UD, its analytic gradient (no mean correction) against autograd and a central difference,
all factors 0 against the oracle's unguided evaluation, a factor changing every style layer -, the binding table, the host-side argument
checks of the four entry points, the refusals of the modules and the preset keys on their way into the modules."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

import flip_restatement as fr
import synth
from conftest import REPO, make_cfg, rel_l2

NAMES = ["maua_gram_flip_bwd", "maua_gram_flip_fwd", "maua_gram_flip_supported", "maua_gram_flip_workspace_bytes"]
KINDS = (fr.LR, fr.UD, fr.ROT180)


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


@pytest.mark.parametrize("cov", [False, True])
@pytest.mark.parametrize("shape", [(7, 9, 13), (3, 5, 7), (2, 1, 6), (2, 6, 1), (1, 1, 1)])
def test_flip_equals_the_index_form_and_is_symmetric(shape, cov):
    f = torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for kind in KINDS:
        a, b = fr.mirrored_gram(f, kind, cov), fr.mirrored_gram_flat(f, kind, cov)
        assert (a - b).abs().max() <= 1e-14 * max(1.0, float(a.abs().max())), kind
        assert (a - a.t()).abs().max() <= 1e-15 * max(1.0, float(a.abs().max())), kind  # symmetric up to the order of the sum


@pytest.mark.parametrize("cov", [False, True])
def test_mirrors_of_a_degenerate_axis_are_the_plain_gram(cov):
    gen = torch.Generator().manual_seed(2)
    for shape, kind in (((4, 9, 1), fr.LR), ((4, 1, 9), fr.UD)):
        f = torch.randn(*shape, dtype=torch.float64, generator=gen)
        x = fr.centred(f, cov).reshape(shape[0], -1)
        assert torch.equal(fr.mirrored_gram(f, kind, cov), x @ x.t() / f.nelement())
        assert torch.equal(fr.mirrored_gram_flat(f, kind, cov), x @ x.t() / f.nelement())


def test_the_point_mirror_is_lr_after_ud():
    H, W = 5, 7
    lr, ud, rot = (fr.sigma(k, H, W) for k in KINDS)
    assert torch.equal(lr[ud], rot) and torch.equal(ud[lr], rot)
    for s in (lr, ud, rot):
        assert torch.equal(s[s], torch.arange(H * W))  # an involution
    f = torch.randn(3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    both = torch.flip(torch.flip(f, (1,)), (2,)).reshape(3, -1) @ f.reshape(3, -1).t() / f.nelement()
    assert torch.equal(fr.mirrored_gram(f, fr.ROT180), both)


@pytest.mark.parametrize("cov", [False, True])
def test_analytic_gradient_equals_autograd_and_a_central_difference(cov):
    """flip_backward subtracts no row mean: with covariance this is the claim that the term through mu vanishes."""
    gen = torch.Generator().manual_seed(4)
    f = torch.randn(7, 9, 13, dtype=torch.float64, generator=gen).requires_grad_(True)
    kinds = [fr.LR, fr.UD, fr.ROT180, fr.LR]
    w = [torch.randn(7, 7, dtype=torch.float64, generator=gen) for _ in kinds]  # not symmetric

    def value(t):
        return sum((fr.mirrored_gram(t, k, cov) * wi).sum() for k, wi in zip(kinds, w))

    value(f).backward()
    want = fr.flip_backward(f.detach(), kinds, w, cov)
    assert rel_l2(want, f.grad) <= 1e-13
    if cov:
        assert float(want.sum((1, 2)).abs().max()) <= 1e-12 * float(want.abs().max()) * 9 * 13  # its rows sum to zero by themselves
    direction = torch.randn(f.shape, dtype=torch.float64, generator=gen)
    h = 1e-5
    fd = (value(f.detach() + h * direction) - value(f.detach() - h * direction)) / (2 * h)
    assert abs(float(fd) - float((f.grad * direction).sum())) <= 1e-8 * abs(float(fd))


@pytest.mark.parametrize("over", [dict(), dict(use_covariance=True), dict(normalize_gradients=False, video_style_factor=0.0)],
                         ids=["default", "covariance", "plain"])
def test_all_factors_zero_is_the_unguided_evaluation(over):
    from oracle.style_oracle import OracleNet, build_spec
    cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", flip_factor=0.0, rotation_factor=0.0, **over)
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    onet = OracleNet(build_spec(cfg), sd, torch.float64)
    onet.capture_content(content)
    onet.capture_style([style], cfg.style_blend_weights)
    total_o, losses_o, grad_o = onet.feval(init)
    net = fr.build(content, [style], cfg, sd)
    assert net.kinds == [] and net.flip_targets == {}
    total, losses, grad = net.feval(init)
    assert sorted(losses) == sorted(losses_o)
    for i in losses:
        assert abs(float(losses[i]) - float(losses_o[i])) <= 1e-12 * abs(float(losses_o[i]))
    assert abs(float(total) - float(total_o)) <= 1e-12 * abs(float(total_o))
    assert rel_l2(grad, grad_o) <= 1e-12


@pytest.mark.parametrize("factors", [dict(flip_factor=0.5), dict(rotation_factor=0.5)], ids=["flip", "rotation"])
def test_a_factor_changes_the_loss_of_every_style_layer(factors):
    """Unlike the shift terms, which need 32 pixels: at 24 x 24 the layers are 24, 12 and 6 pixels wide and all three terms grow."""
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    vals = {}
    for on in (False, True):
        cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", video_style_factor=0.0, normalize_gradients=False,
                       **(factors if on else {}))
        net = fr.build(content, [style], cfg, sd)
        vals[on] = (net, net.feval(init)[1])
    net = vals[True][0]
    assert net.kinds == ([fr.LR, fr.UD] if "flip_factor" in factors else [fr.ROT180])
    style_slots = [i for i, l in enumerate(net.spec) if l.kind == "style"]
    assert len(style_slots) == 3
    for i in style_slots:
        assert float(vals[True][1][i]) > float(vals[False][1][i]), i
    for i in vals[False][1]:
        if i not in style_slots:
            assert float(vals[True][1][i]) == float(vals[False][1][i])


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_gram_flip_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if n.startswith("maua_gram_flip_")) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("gram_flip_supported", "gram_flip_workspace_bytes", "gram_flip_fwd", "gram_flip_bwd"))
    assert hip.lib().maua_abi_version() == 2


def test_refused_shapes_answer_zero_without_a_gpu(libpath):
    import hip
    L = hip.lib()
    assert L.maua_gram_flip_supported(1, 64, 32, 32) == 1 and L.maua_gram_flip_workspace_bytes(1, 64, 32, 32) > 0
    assert L.maua_gram_flip_supported(4, 1, 1, 1) == 1 and L.maua_gram_flip_supported(1, 65536, 1, (1 << 30) - 1) == 1
    for mirrors, c, h, w in ((0, 64, 32, 32), (5, 64, 32, 32), (-1, 64, 32, 32), (1, 0, 32, 32), (1, 65537, 32, 32), (1, 64, -32, 32),
                             (1, 64, 32, -32), (1, 64, -32, -32), (1, 64, 0, 32), (1, 64, 32, 0), (1, 64, 1 << 15, 1 << 15),
                             (1, 64, 2147483647, 2147483647)):
        assert L.maua_gram_flip_supported(mirrors, c, h, w) == 0, (mirrors, c, h, w)
        assert L.maua_gram_flip_workspace_bytes(mirrors, c, h, w) == 0, (mirrors, c, h, w)
    # the split of the plane does not depend on the number of mirrors; only the tile pairs on or above the diagonal have slabs
    one = L.maua_gram_flip_workspace_bytes(1, 130, 20, 35)
    assert L.maua_gram_flip_workspace_bytes(3, 130, 20, 35) == 3 * one
    assert one % (6 * 64 * 64 * 4) == 0  # three channel tiles: six pairs


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: MAUA_E_INVAL (-1).  0 or 5 mirrors, a kind outside {0, 1, 2}, h w >= 2^30: MAUA_E_UNSUPPORTED (-2).  A workspace one
    byte short: MAUA_E_WORKSPACE (-3).  All before any launch - the pointers handed over here are host memory no kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_float * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    one = (ctypes.c_double * 1)(1.0)
    five = (ctypes.c_double * 5)()
    big = 1 << 30
    assert L.maua_gram_flip_fwd(None, None, None, None, None, 1, 3, 5, 7, None, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_gram_flip_bwd(None, None, None, None, None, None, 1, 3, 5, 7, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_gram_flip_fwd(ptr, None, ints(0), one, None, 1, 3, 5, 7, ptr, big, None) == -1   # gram
    assert L.maua_gram_flip_fwd(ptr, None, None, one, ptr, 1, 3, 5, 7, ptr, big, None) == -1       # kinds
    assert L.maua_gram_flip_fwd(ptr, None, ints(0), one, ptr, 1, 3, 5, 7, None, big, None) == -1   # workspace
    assert L.maua_gram_flip_bwd(ptr, ptr, None, ints(0), one, None, 1, 3, 5, 7, 0, None) == -1     # gx
    assert L.maua_gram_flip_bwd(ptr, ptr, None, ints(0), None, ptr, 1, 3, 5, 7, 0, None) == -1     # coefs
    for mirrors in (0, 5, -1):
        assert L.maua_gram_flip_fwd(ptr, None, ints(0, 1, 2, 0, 1), five, ptr, mirrors, 3, 5, 7, ptr, big, None) == -2, mirrors
        assert b"mirrors" in L.maua_last_error()
        assert L.maua_gram_flip_bwd(ptr, ptr, None, ints(0, 1, 2, 0, 1), five, ptr, mirrors, 3, 5, 7, 0, None) == -2, mirrors
    for kind in (3, -1):
        assert L.maua_gram_flip_fwd(ptr, None, ints(0, kind), five, ptr, 2, 3, 5, 7, ptr, big, None) == -2, kind
        assert b"kind" in L.maua_last_error()
        assert L.maua_gram_flip_bwd(ptr, ptr, None, ints(0, kind), five, ptr, 2, 3, 5, 7, 0, None) == -2, kind
        assert b"kind" in L.maua_last_error()
    for h, w in ((1 << 15, 1 << 15), (1, 1 << 30), (0, 7), (5, 0)):
        assert L.maua_gram_flip_fwd(ptr, None, ints(0), one, ptr, 1, 3, h, w, ptr, big, None) == -2, (h, w)
        assert L.maua_gram_flip_bwd(ptr, ptr, None, ints(0), one, ptr, 1, 3, h, w, 0, None) == -2, (h, w)
    for c in (0, 65537):
        assert L.maua_gram_flip_fwd(ptr, None, ints(0), one, ptr, 1, c, 5, 7, ptr, big, None) == -2, c
    need = L.maua_gram_flip_workspace_bytes(2, 3, 5, 7)
    assert need > 0
    assert L.maua_gram_flip_fwd(ptr, None, ints(0, 2), five, ptr, 2, 3, 5, 7, ptr, need - 1, None) == -3  # one byte short
    assert b"workspace" in L.maua_last_error()


def test_gram_matrix_refuses_a_flip_with_a_shift_and_flipped_batches():
    import loss
    g = loss.GramMatrix()
    for kw in (dict(flip_h=True, shift_x=4), dict(flip_v=True, shift_y=4), dict(flip_h=True, flip_v=True, shift_x=4)):
        with pytest.raises(ValueError, match="a flip and a shift"):
            g(torch.zeros(1, 3, 8, 8), **kw)
    with pytest.raises(ValueError, match="one frame"):
        g(torch.zeros(2, 3, 8, 8), flip_h=True)


@pytest.mark.parametrize("factors", [dict(flip_factor=0.5), dict(rotation_factor=0.5)], ids=["flip", "rotation"])
def test_a_guided_module_with_a_mirror_factor_raises(factors):
    import loss
    m = loss.StyleLoss(1.0, **factors)
    assert m.flip_targets == {}
    m._guide = torch.ones(1, 8, 8)
    m.mode = "loss"
    with pytest.raises(NotImplementedError, match="flip_factor / rotation_factor"):
        m(torch.zeros(1, 3, 8, 8))


def test_mirror_kinds_follow_the_factors_and_reset_clears_the_targets():
    import loss
    assert loss.StyleLoss(1.0).mirror_kinds() == []
    assert loss.StyleLoss(1.0, flip_factor=1.0).mirror_kinds() == [0, 1]
    assert loss.StyleLoss(1.0, rotation_factor=1.0).mirror_kinds() == [2]
    m = loss.StyleLoss(1.0, flip_factor=1.0, rotation_factor=0.5)
    assert m.mirror_kinds() == [0, 1, 2]
    m.flip_targets[0] = torch.zeros(3, 3)
    m.reset_targets()
    assert m.flip_targets == {}


def test_engine_and_optim_divert_a_mirrored_module():
    import engine
    import loss
    import optim
    for factors in (dict(flip_factor=0.5), dict(rotation_factor=0.5)):
        m = loss.StyleLoss(1.0, **factors)
        assert optim._mirrored([m]) and not optim._shifted([m]) and not optim._mirrored([loss.StyleLoss(1.0, shift_factor=1.0)])
        with pytest.raises(engine.UnsupportedNet, match="mirrored StyleLoss runs on the module path"):
            engine.StyleEngine(torch.nn.Sequential(m), [m])
        net = torch.nn.Sequential(m)
        net.style_losses = [m]
        assert optim._engine_of(net) is None and not getattr(net, "_maua_engine_refused", False)


def test_frame_batches_of_a_mirrored_net_fall_back_to_one_frame_per_call():
    """optimize_frames refuses a mirrored network before anything runs, which style._optimize_group turns into one optim.optimize call per
    frame - the fallback of a shifted network."""
    import engine
    import loss
    import optim
    m = loss.StyleLoss(1.0, flip_factor=1.0)
    net = torch.nn.Sequential(m)
    net.style_losses = [m]
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(engine.UnsupportedNet, match="frame batches"):
        optim.optimize_frames(x, [x[:1]], x, 1, None, net, [m])
    assert optim._style_targets_missing(net)
    m.target = torch.zeros(3, 3)
    assert optim._style_targets_missing(net)  # (the static target alone does not do: a factor switched on after a capture)
    m.flip_targets = {0: torch.zeros(3, 3), 1: torch.zeros(3, 3)}
    assert not optim._style_targets_missing(net)
    m.rotation_factor = 0.5
    assert optim._style_targets_missing(net)


def test_preset_keys_reach_the_modules(tmp_path):
    """The factors are no flags (the flag surface is the reference's): they arrive through --load_args, as content_mask does."""
    import config
    preset = tmp_path / "sym.json"
    preset.write_text(json.dumps({"flip_factor": 1.0, "rotation_factor": 0.5}))
    args = config.get_args(["--content", "c.png", "--style", "s.png", "--load_args", str(preset)])
    assert args.flip_factor == 1.0 and args.rotation_factor == 0.5
    assert not any(flag in ("flip_factor", "rotation_factor") for flag, _ in config._FLAGS)
    plain = config.get_args(["--content", "c.png", "--style", "s.png"])
    assert not hasattr(plain, "flip_factor")

    import models
    for a, want in ((args, (1.0, 0.5)), (plain, (0.0, 0.0))):
        cnn = models.VGG(models.build_sequential(models.channel_list["VGG-19"], a.pooling))
        net, _ = models.assemble(cnn.features, models.vgg19_dict, a)
        assert len(net.style_losses) == 5
        assert all((m.flip_factor, m.rotation_factor) == want for m in net.style_losses)
        assert all(m.mirror_kinds() == ([0, 1, 2] if want[0] else []) for m in net.style_losses)
