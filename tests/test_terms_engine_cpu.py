"""Host side of the shift and mirror terms on the fused engine (StyleLoss.terms_engine): engine.term_coefficients against fp64 autograd over a
literal restatement of the scalar arithmetic of loss.StyleLoss.static_loss, the six entry points in the header and the binding table, the
answers of the two *_supported functions, the host-side argument checks, and the switch's default.  No GPU."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO

NAMES = ["maua_flip_gram_bwd_masked", "maua_flip_gram_fwd_mse_ledger", "maua_flip_gram_mse_ledger_supported",
         "maua_shift_gram_bwd_masked", "maua_shift_gram_fwd_mse_ledger", "maua_shift_gram_mse_ledger_supported"]


@pytest.fixture(scope="module")
def libpath():
    import build_native
    return build_native.build()


class ScaleGradients(torch.autograd.Function):
    """loss.ScaleGradients, restated: identity forwards, g -> g / (|g| + 1e-8) * strength^2 backwards."""

    @staticmethod
    def forward(ctx, input_tensor, strength):
        ctx.strength = strength
        return input_tensor

    @staticmethod
    def backward(ctx, grad_output):
        unit = grad_output / (torch.norm(grad_output, keepdim=True) + 1e-8)
        return unit * ctx.strength * ctx.strength, None


def static_loss64(gram, target, grams, targets, factors, strength, normalize):
    """static_loss for one frame: t = mse(G, T) + sum_k factor_k mse(G_k, T_k), through ScaleGradients with `normalize`, times the strength."""
    t = ((gram - target) ** 2).mean()
    for k, factor in enumerate(factors):
        t = t + factor * ((grams[k] - targets[k]) ** 2).mean()
    if normalize:
        t = ScaleGradients.apply(t, strength)
    return t * strength


@pytest.mark.parametrize("normalize,factors", list(itertools.product([False, True], [[1.0], [0.5, 0.5, 2.0, 2.0], [3.0, 0.0, 0.25], []])))
def test_coefficients_reproduce_static_loss(normalize, factors):
    import engine
    C, strength = 7, 0.37
    K = len(factors)
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    gram, target = rnd(C, C).requires_grad_(True), rnd(C, C)
    grams, targets = rnd(K, C, C).requires_grad_(True), rnd(K, C, C)  # (not symmetric: a shifted product is not)
    loss = static_loss64(gram, target, grams, targets, factors, strength, normalize)
    ls, gs = engine.term_coefficients(strength, normalize, C, factors)
    assert len(ls) == len(gs) == K
    # the plain term's weights of the engine: no dynamic term here (video_style_factor 0)
    lw = strength
    gw = engine._scale_grad_coeff(strength, strength) if normalize else strength
    diff = (grams - targets).detach()
    want_loss = lw / C ** 2 * float(((gram - target).detach() ** 2).sum()) + sum(ls[k] * float((diff[k] ** 2).sum()) for k in range(K))
    assert abs(float(loss.detach()) - want_loss) <= 1e-12 * abs(want_loss)
    dg0, dg = torch.autograd.grad(loss, [gram, grams], allow_unused=True)
    want0 = gw * 2.0 / C ** 2 * (gram - target).detach()
    assert float((dg0 - want0).norm()) <= 1e-12 * float(want0.norm())
    for k in range(K):
        want = gs[k] * diff[k]  # dL/dG_k as it is: the backward kernels add the transpose themselves
        if factors[k] == 0:
            assert ls[k] == 0.0 and gs[k] == 0.0 and not bool(dg[k].any())
            continue
        assert float((dg[k] - want).norm()) <= 1e-12 * float(want.norm()), (k, normalize)


def test_header_signatures_and_exported_symbols_agree(libpath):
    import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "maua_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(maua_(?:shift|flip)_gram_[a-z0-9_]+)\s*\(", header)))
    assert declared == NAMES
    assert sorted(n for n in hip.SIGNATURES if re.match(r"maua_(shift|flip)_gram_", n)) == NAMES
    for name in NAMES:  # argument counts of the binding = parameter counts of the declaration
        params = re.search(name + r"\s*\(([^()]*)\)\s*;", header).group(1).split(",")
        assert len(hip.SIGNATURES[name][1]) == len(params), name
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", exported), name
    assert all(callable(getattr(hip, n)) for n in ("gram_shift_fwd_mse_ledger", "gram_shift_bwd_masked", "gram_shift_mse_ledger_supported",
                                                   "gram_flip_fwd_mse_ledger", "gram_flip_bwd_masked", "gram_flip_mse_ledger_supported"))
    assert hip.lib().maua_abi_version() == 2


def test_supported_answers_follow_the_record(libpath):
    """16, 8 or 4 partial sums per (term, tile pair) - the most that fit 4096: shifts over all nt^2 pairs, mirrors over nt (nt + 1) / 2."""
    import hip
    L = hip.lib()
    shift, flip = L.maua_shift_gram_mse_ledger_supported, L.maua_flip_gram_mse_ledger_supported
    for c in (64, 128, 256, 512):  # VGG-19: at most 4 shifts ([4, 16] along x and y) on the layers of up to 512 channels, 3 mirrors
        assert shift(4, c) == 1 and flip(3, c) == 1, c
    assert shift(1, 1) == 1 and shift(16, 512) == 1 and flip(4, 1408) == 1 and shift(1, 2048) == 1
    assert shift(16, 513) == 0 and shift(1, 2049) == 0 and shift(4, 1025) == 0  # 16 x 81 x 4, 1 x 33^2 x 4, 4 x 17^2 x 4 > 4096
    assert flip(4, 1409) == 0 and flip(1, 2881) == 0  # 4 x 23 x 24 / 2 x 4, 1 x 46 x 47 / 2 x 4 > 4096
    for terms, c in ((0, 64), (-1, 64), (17, 64), (1, 0), (1, 65537)):
        assert shift(terms, c) == 0, (terms, c)
    for terms, c in ((0, 64), (-1, 64), (5, 64), (1, 0), (1, 65537)):
        assert flip(terms, c) == 0, (terms, c)


def test_invalid_arguments_are_rejected_without_touching_the_gpu(libpath):
    """Null pointers: MAUA_E_INVAL (-1).  Unsupported counts, axes, deltas, kinds, shapes, or a record that does not fit: MAUA_E_UNSUPPORTED
    (-2).  A workspace one byte short: MAUA_E_WORKSPACE (-3).  All before any launch - the pointers handed over here are host memory no
    kernel could use."""
    import hip
    L = hip.lib()
    host = (ctypes.c_float * 16)()
    ptr = ctypes.cast(host, ctypes.c_void_p)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    dbl = lambda n: (ctypes.c_double * n)(*([1.0] * n))
    big = 1 << 30
    sf, sb = L.maua_shift_gram_fwd_mse_ledger, L.maua_shift_gram_bwd_masked
    ff, fb = L.maua_flip_gram_fwd_mse_ledger, L.maua_flip_gram_bwd_masked

    def shift_fwd(f=ptr, axes=ints(0), deltas=ints(4), scales=dbl(1), gram=ptr, shifts=1, c=3, h=5, w=7, target=ptr, ls=dbl(1), gs=dbl(1),
                  dmat=ptr, ledger=ptr, slot=0, ws=ptr, ws_bytes=big):
        return sf(f, None, axes, deltas, scales, gram, shifts, c, h, w, target, ls, gs, dmat, ledger, slot, ws, ws_bytes, None)

    def flip_fwd(f=ptr, kinds=ints(0), scales=dbl(1), gram=ptr, mirrors=1, c=3, h=5, w=7, target=ptr, ls=dbl(1), gs=dbl(1), dmat=ptr,
                 ledger=ptr, slot=0, ws=ptr, ws_bytes=big):
        return ff(f, None, kinds, scales, gram, mirrors, c, h, w, target, ls, gs, dmat, ledger, slot, ws, ws_bytes, None)

    for fwd, nullable in ((shift_fwd, ("f", "axes", "deltas", "scales", "gram", "target", "ls", "gs", "dmat", "ledger", "ws")),
                          (flip_fwd, ("f", "kinds", "scales", "gram", "target", "ls", "gs", "dmat", "ledger", "ws"))):
        for name in nullable:
            assert fwd(**{name: None}) == -1, name
        assert fwd(slot=-1) == -1
    assert sb(None, None, None, None, None, None, None, None, 1, 3, 5, 7, 0, None) == -1 and b"null" in L.maua_last_error()
    assert fb(None, None, None, None, None, None, None, 1, 3, 5, 7, 0, None) == -1 and b"null" in L.maua_last_error()
    assert sb(ptr, ptr, None, ints(0), ints(4), dbl(1), ptr, None, 1, 3, 5, 7, 0, None) == -1  # gx (the mask alone may be null)
    assert fb(ptr, ptr, None, ints(0), dbl(1), ptr, None, 1, 3, 5, 7, 0, None) == -1           # gx
    assert sb(ptr, ptr, None, ints(0), ints(4), None, ptr, ptr, 1, 3, 5, 7, 0, None) == -1     # coefs
    assert fb(ptr, ptr, None, ints(0), None, ptr, ptr, 1, 3, 5, 7, 0, None) == -1              # coefs

    for shifts in (0, 17, -1):
        assert shift_fwd(axes=ints(*[0] * 17), deltas=ints(*[1] * 17), scales=dbl(17), ls=dbl(17), gs=dbl(17), shifts=shifts) == -2, shifts
        assert b"shifts" in L.maua_last_error()
        assert sb(ptr, ptr, None, ints(*[0] * 17), ints(*[1] * 17), dbl(17), ptr, ptr, shifts, 3, 5, 7, 0, None) == -2, shifts
    for axis, delta in ((2, 1), (-1, 1), (0, 0), (0, 7), (1, 5), (0, -1)):
        assert shift_fwd(axes=ints(axis), deltas=ints(delta)) == -2, (axis, delta)
        assert sb(ptr, ptr, None, ints(axis), ints(delta), dbl(1), ptr, ptr, 1, 3, 5, 7, 0, None) == -2, (axis, delta)
    for mirrors in (0, 5, -1):
        assert flip_fwd(kinds=ints(0, 1, 2, 0, 1), scales=dbl(5), ls=dbl(5), gs=dbl(5), mirrors=mirrors) == -2, mirrors
        assert b"mirrors" in L.maua_last_error()
        assert fb(ptr, ptr, None, ints(0, 1, 2, 0, 1), dbl(5), ptr, ptr, mirrors, 3, 5, 7, 0, None) == -2, mirrors
    for kind in (3, -1):
        assert flip_fwd(kinds=ints(0, kind), scales=dbl(2), ls=dbl(2), gs=dbl(2), mirrors=2) == -2 and b"kind" in L.maua_last_error()
        assert fb(ptr, ptr, None, ints(0, kind), dbl(2), ptr, ptr, 2, 3, 5, 7, 0, None) == -2 and b"kind" in L.maua_last_error()
    for h, w in ((1 << 15, 1 << 15), (0, 7), (5, 0)):
        assert shift_fwd(h=h, w=w) == -2 and flip_fwd(h=h, w=w) == -2, (h, w)
        assert sb(ptr, ptr, None, ints(0), ints(4), dbl(1), ptr, ptr, 1, 3, h, w, 0, None) == -2, (h, w)
        assert fb(ptr, ptr, None, ints(0), dbl(1), ptr, ptr, 1, 3, h, w, 0, None) == -2, (h, w)
    for c in (0, 65537):
        assert shift_fwd(c=c) == -2 and flip_fwd(c=c) == -2, c
    # a record that does not fit: -2, even with a workspace far too small for the shape (the check comes first)
    assert shift_fwd(c=2049, ws_bytes=16) == -2 and b"partial sums" in L.maua_last_error()
    assert flip_fwd(c=2881, ws_bytes=16) == -2 and b"partial sums" in L.maua_last_error()
    need = L.maua_gram_shift_workspace_bytes(1, 3, 5, 7)
    assert need > 0 and shift_fwd(ws_bytes=need - 1) == -3 and b"workspace" in L.maua_last_error()
    need = L.maua_gram_flip_workspace_bytes(1, 3, 5, 7)
    assert need > 0 and flip_fwd(ws_bytes=need - 1) == -3 and b"workspace" in L.maua_last_error()


def test_the_switch_defaults_to_the_module_path():
    import loss
    import optim
    import plan

    assert loss.StyleLoss(1.0).terms_engine is False
    assert "terms_engine" not in plan.FIELDS  # a per-network switch (preset key), not a planner field

    class Net:
        pass

    for kw in (dict(shift_factor=1.0), dict(flip_factor=1.0), dict(rotation_factor=1.0)):
        net = Net()
        net.style_losses = [loss.StyleLoss(1.0, **kw)]
        assert optim._engine_of(net) is None
        assert not hasattr(net, "_maua_engine") and not getattr(net, "_maua_engine_refused", False)  # (not remembered)
        assert optim._terms_on_module_path(net) is not None
        net.style_losses[0].terms_engine = True
        assert optim._terms_on_module_path(net) is None and (optim._shifted(net) or optim._mirrored(net))
