"""Shifted-Gram style loss without a GPU: loss.shift_deltas against the table of the definition, the fp64 restatement
(tests/shift_restatement.py) - slices against the flat-offset form, its analytic gradient against autograd and a central difference, and
shift_factor = 0 against the oracle's unguided evaluation -, the binding table, the host-side argument checks of the four entry points, and the
refusals of the modules."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import shift_restatement as sr
import synth
from conftest import REPO, make_cfg, rel_l2

NAMES = ["maua_gram_shift_bwd", "maua_gram_shift_fwd", "maua_gram_shift_supported", "maua_gram_shift_workspace_bytes"]


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


def table(n):
    if n < 32:
        return []
    if n < 128:
        return [4]
    if n < 512:
        return [4, 16]
    if n < 2048:
        return [4, 16, 64]
    return [4, 16, 64, 256]


def test_shift_deltas_follow_the_table():
    import loss
    for n in range(8, 2049):
        assert loss.shift_deltas(n, n) == table(n), n
        assert sr.deltas(n) == table(n), n
        assert all(d <= n // 8 for d in table(n))
    assert loss.shift_deltas(40, 2000) == [4] and loss.shift_deltas(2000, 40) == [4] and loss.shift_deltas(16, 16) == []


@pytest.mark.parametrize("cov", [False, True])
def test_slices_equal_the_flat_offset_form(cov):
    f = torch.randn(7, 9, 13, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for axis, d in ((0, 1), (0, 4), (0, 12), (1, 1), (1, 4), (1, 8)):
        a, b = sr.shifted_gram(f, axis, d, cov), sr.shifted_gram_flat(f, axis, d, cov)
        assert rel_l2(a, b) <= 1e-14, (axis, d)
        assert rel_l2(a, a.t()) > 1e-3  # (not symmetric)


@pytest.mark.parametrize("cov", [False, True])
def test_analytic_gradient_equals_autograd_and_a_central_difference(cov):
    gen = torch.Generator().manual_seed(2)
    f = torch.randn(7, 9, 13, dtype=torch.float64, generator=gen).requires_grad_(True)
    shifts = [(0, 4), (1, 4), (0, 1), (1, 8)]
    w = [torch.randn(7, 7, dtype=torch.float64, generator=gen) for _ in shifts]

    def value(t):
        return sum((sr.shifted_gram(t, a, d, cov) * wi).sum() for (a, d), wi in zip(shifts, w))

    value(f).backward()
    want = sr.shift_backward(f.detach(), shifts, w, cov)
    assert rel_l2(want, f.grad) <= 1e-13
    direction = torch.randn(f.shape, dtype=torch.float64, generator=gen)
    h = 1e-5
    fd = (value(f.detach() + h * direction) - value(f.detach() - h * direction)) / (2 * h)
    assert abs(float(fd) - float((f.grad * direction).sum())) <= 1e-8 * abs(float(fd))


@pytest.mark.parametrize("over", [dict(), dict(use_covariance=True), dict(normalize_gradients=False, video_style_factor=0.0)],
                         ids=["default", "covariance", "plain"])
def test_shift_factor_zero_is_the_unguided_evaluation(over):
    from oracle.style_oracle import OracleNet, build_spec
    cfg = make_cfg(style_layers="relu1_1,relu2_1,relu3_1", content_layers="relu2_2", **over)
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(24))
    onet = OracleNet(build_spec(cfg), sd, torch.float64)
    onet.capture_content(content)
    onet.capture_style([style], cfg.style_blend_weights)
    total_o, losses_o, grad_o = onet.feval(init)
    net = sr.build(content, [style], cfg, sd)
    total, losses, grad = net.feval(init)
    assert sorted(losses) == sorted(losses_o)
    for i in losses:
        assert abs(float(losses[i]) - float(losses_o[i])) <= 1e-12 * abs(float(losses_o[i]))
    assert abs(float(total) - float(total_o)) <= 1e-12 * abs(float(total_o))
    assert rel_l2(grad, grad_o) <= 1e-12


def test_a_shift_factor_changes_the_layers_that_have_deltas():
    """At 40 x 40 relu1_1 (40) has delta 4 and relu2_1 (20) none: the first style term grows, the second keeps its value."""
    sd = synth.vgg19_state_dict(dtype=torch.float64)
    content, style, init = (t.double() for t in synth.images(40))
    vals = {}
    for sf in (0.0, 0.5):
        cfg = make_cfg(style_layers="relu1_1,relu2_1", content_layers="relu2_2", shift_factor=sf)
        net = sr.build(content, [style], cfg, sd)
        vals[sf] = (net, net.feval(init)[1])
    net = vals[0.5][0]
    first, second = [i for i, l in enumerate(net.spec) if l.kind == "style"]
    assert net.shift_deltas == {first: [4], second: []}
    assert float(vals[0.5][1][first]) > float(vals[0.0][1][first])
    assert float(vals[0.5][1][second]) == float(vals[0.0][1][second])


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_gram_shift_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if n.startswith("maua_gram_shift_")) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("gram_shift_supported", "gram_shift_workspace_bytes", "gram_shift_fwd", "gram_shift_bwd"))


def test_refused_shapes_answer_zero_without_a_gpu(libpath):
    import hip
    L = hip.lib()
    assert L.maua_gram_shift_supported(1, 64, 32, 32) == 1 and L.maua_gram_shift_workspace_bytes(1, 64, 32, 32) > 0
    assert L.maua_gram_shift_supported(16, 1, 1, 2) == 1
    for shifts, c, h, w in ((0, 64, 32, 32), (17, 64, 32, 32), (-1, 64, 32, 32), (1, 0, 32, 32), (1, 65537, 32, 32), (1, 64, -32, 32),
                            (1, 64, 32, -32), (1, 64, -32, -32), (1, 64, 0, 32), (1, 64, 1 << 15, 1 << 15), (1, 64, 2147483647, 2147483647)):
        assert L.maua_gram_shift_supported(shifts, c, h, w) == 0, (shifts, c, h, w)
        assert L.maua_gram_shift_workspace_bytes(shifts, c, h, w) == 0, (shifts, c, h, w)
    # the split of the plane does not depend on the number of shifts
    one = L.maua_gram_shift_workspace_bytes(1, 130, 20, 35)
    assert L.maua_gram_shift_workspace_bytes(4, 130, 20, 35) == 4 * one


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: -1.  A delta of 0, a delta of the axis extent, an axis that is neither x nor y: MAUA_E_UNSUPPORTED (-2), before any
    launch - the pointers handed over here are host memory no kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_float * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    one = (ctypes.c_double * 1)(1.0)
    assert L.maua_gram_shift_fwd(None, None, None, None, None, None, 1, 3, 5, 7, None, 0, None) == -1
    assert b"null" in L.maua_last_error()
    assert L.maua_gram_shift_bwd(None, None, None, None, None, None, None, 1, 3, 5, 7, 0, None) == -1
    assert L.maua_gram_shift_fwd(ptr, None, ints(0), ints(4), one, None, 1, 3, 5, 7, ptr, 1 << 20, None) == -1   # gram
    assert L.maua_gram_shift_bwd(ptr, ptr, None, ints(0), ints(4), one, None, 1, 3, 5, 7, 0, None) == -1          # gx
    for axis, delta in ((0, 0), (0, 7), (1, 5), (1, 0), (0, -1), (1, 6), (2, 1), (-1, 1)):
        assert L.maua_gram_shift_fwd(ptr, None, ints(axis), ints(delta), one, ptr, 1, 3, 5, 7, ptr, 1 << 20, None) == -2, (axis, delta)
        assert b"shift" in L.maua_last_error()
        assert L.maua_gram_shift_bwd(ptr, ptr, None, ints(axis), ints(delta), one, ptr, 1, 3, 5, 7, 0, None) == -2, (axis, delta)
    for shifts in (0, 17):
        assert L.maua_gram_shift_fwd(ptr, None, ints(*[0] * 17), ints(*[1] * 17), (ctypes.c_double * 17)(), ptr, shifts, 3, 5, 7, ptr, 1 << 20,
                                     None) == -2
    assert L.maua_gram_shift_fwd(ptr, None, ints(0), ints(4), one, ptr, 1, 3, 5, 7, ptr, 16, None) == -3  # workspace too small


def test_gram_matrix_refuses_two_shifts_and_shifted_batches():
    import loss
    g = loss.GramMatrix()
    with pytest.raises(ValueError, match="one of shift_x / shift_y"):
        g(torch.zeros(1, 3, 8, 8), shift_x=4, shift_y=4)
    with pytest.raises(ValueError, match="one frame"):
        g(torch.zeros(2, 3, 8, 8), shift_x=4)


def test_a_guided_module_with_a_shift_factor_raises():
    import loss
    m = loss.StyleLoss(1.0, shift_factor=0.5)
    assert m.shift_targets_x == [] and m.shift_targets_y == [] and m.shift_target_deltas is None
    m._guide = torch.ones(1, 8, 8)
    m.mode = "loss"
    with pytest.raises(NotImplementedError, match="shift_factor"):
        m(torch.zeros(1, 3, 8, 8))


def test_engine_and_optim_divert_a_shifted_module():
    import engine
    import loss
    import optim
    m = loss.StyleLoss(1.0, shift_factor=0.5)
    assert optim._shifted([m]) and not optim._shifted([loss.StyleLoss(1.0)])
    with pytest.raises(engine.UnsupportedNet, match="shifted StyleLoss runs on the module path"):
        engine.StyleEngine(torch.nn.Sequential(m), [m])
    net = torch.nn.Sequential(m)
    net.style_losses = [m]
    assert optim._engine_of(net) is None and not getattr(net, "_maua_engine_refused", False)


def test_frame_batches_of_a_shifted_net_fall_back_to_one_frame_per_call():
    """vid_img's independent frame batches need the engine: optimize_frames refuses a shifted network before anything runs, which is what
    style._optimize_group turns into one optim.optimize call per frame."""
    import engine
    import loss
    import optim
    m = loss.StyleLoss(1.0, shift_factor=1.0)
    net = torch.nn.Sequential(m)
    net.style_losses = [m]
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(engine.UnsupportedNet, match="frame batches"):
        optim.optimize_frames(x, [x[:1]], x, 1, None, net, [m])
    assert optim._style_targets_missing(net)
