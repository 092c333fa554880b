"""Every tuning constant of libmaua_hip (the "lib" fields of plan.FIELDS, what MAUA_PLAN="field=value" sets and tools/ab_*.sh compare) at
its NON-default values, against plain fp64 on the CPU.

The other GPU modules are thorough at the defaults; behind most of the switches sits a second kernel, a second template instantiation or
a second derivation of the order in which workgroups walk their work, and an A/B number measured through a wrong one decides the next
default.  `VARIANTS` lists the values this module forces, `COVERED_ELSEWHERE` the fields whose forcing tests exist already;
tests/test_host_logic.py checks that the two tables cover plan.FIELDS (a constant added later without a test of its other setting fails
there), so this module imports without a GPU.

How a field is forced: plan.OVERRIDES[field] = value + plan.forward_to_library(lib), in-process.  Every constant is read by
`maua::tuning(name, default)` at the launch (csrc/conv_api.hip: a table lookup, no `static` copy anywhere in csrc/), and the sizes
that depend on one (split-K slabs, the Gram slabs of gram_plan) are asked for AFTER the field is set - the hip.py wrappers size their
workspaces at the call.  The `static` words next to the launches only remember that a kernel's dynamic LDS was opted in.

References: F.conv2d / conv_transpose2d / @ in fp64 on the CPU, oracle.lbfgs_run for the optimiser.  Bars are the ones the modules at
the defaults assert (each named where it is used).  Outputs start as NaN (or as the accumulated-into values): a tile no workgroup
writes fails both the fp64 bar and the bit comparison.  Fields that only reorder or delay work (cot_inner, x3p_order, x3p_groups,
x3w_stagger, p1_order) must leave the bits of the default: a tile's sums are formed by one workgroup in the order of its own chunk
loop whatever tile the workgroup was dealt (conv_x3w.hip:223-229, conv_x3q.hip:179-185, conv_x3p.hip:160-231, conv1x1_x3.hip:60-70);
lbfgs_vec is NOT such a field (see test_lbfgs_scalar_sweeps).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import plan
from conftest import planar_codes, rel_l2

pytestmark = pytest.mark.gpu

BAR = 2e-6        # tests/test_conv_x3w_gpu.py, test_conv_x3q_gpu.py, test_conv_x3p_gpu.py: the fp16x3 convolutions against fp64
TOL = 2e-5        # tests/test_kernels_gpu.py: the fp32 kernels against fp64

# field -> the non-default values this module runs kernels (or routing queries) under
VARIANTS = {
    "cot_inner": (1,),
    "x3p_order": (0,),
    "x3p_ks": (2, 3, 4),
    "x3p_groups": (8, 16, 4),
    "x3w_stagger": (0, 3),
    "conv_few_out": (0,),
    "few_out_ks4_below": (0, 1000000),
    "gram_x3": (0,),
    "gram_bwd_x3": (0,),
    "gram_t128_min_hw": (64,),
    "p1_order": (0,),
    "lbfgs_vec": (0,),
    "lbfgs_tri": (0,),
    "x3q_min_fill": (0, 2.0),
    "x3q_min_chunks": (0, 10 ** 9),
    "x3p_min_fill": (0, 2.0),
    "x3p_min_items": (0, 10 ** 9),
}
# field -> a test that forces it already (this module forces some of them too: ragged x3w_ks / x3q_ks splits, gram_t128 = 2 on small maps)
COVERED_ELSEWHERE = {
    "x3w_ks": "tests/test_finish_in_launch_gpu.py::test_in_launch_finish_equals_the_finishing_launch_bit_for_bit",
    "x3q_ks": "tests/test_finish_in_launch_gpu.py::test_in_launch_finish_equals_the_finishing_launch_bit_for_bit",
    "finish_in_launch_max_ks": "tests/test_finish_in_launch_gpu.py::test_larger_splits_and_other_workspaces_keep_the_finishing_launch",
    "gram_mask_reuse": "tests/test_x3w_gram_mask_gpu.py::test_gram_backward_masks_from_its_own_operand",
    "x6_persist": "tests/test_kernels_gpu.py::test_conv3x3_x6_persistent_workgroups_subprocess",
    "gram_t128": "tests/test_kernels_gpu.py::test_gram_128_blocks_stress_and_the_64_route_subprocess",
}
_FORCED = set(VARIANTS) | {"x3w_ks", "x3q_ks", "gram_t128"}


@pytest.fixture(scope="module")
def hip():
    import hip as h
    h.lib()
    yield h
    h.conv_x3p_set_max_groups(0)


@pytest.fixture(autouse=True)
def _restore(hip):
    yield
    for k in _FORCED:
        plan.OVERRIDES.pop(k, None)
    plan.forward_to_library(hip.lib())
    hip.conv_arm_workspace(None)
    hip.conv_x3p_set_max_groups(0)


def force(hip, **fields):
    for k, v in fields.items():
        assert k in _FORCED
        plan.OVERRIDES[k] = str(v)
    plan.forward_to_library(hip.lib())


def dev(t):
    return t.cuda().contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def nans(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def one_pass_ws():
    """A workspace too small for split-K slabs: the entry point then makes one pass over the channels."""
    return torch.empty(16, dtype=torch.uint8, device="cuda")


def poisoned_ws(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")   # (all-ones words: NaN as floats)


def check(name, got, ref64, bar):
    e = rel_l2(got.cpu(), ref64)
    print(f"{name}: rel_l2 {e:.3e} (bar {bar:.1e})")
    assert e <= bar, name


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs and fp64 references, computed once per geometry
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_case(cin, cout, H, W, n, pad=1):
    """A layer cin -> cout: post-ReLU input, He-scaled filters, bias; conv64 = the fp64 convolution without the bias."""
    s = 131 * cin + 7 * cout + H + W
    x = torch.relu(rnd(n, cin, H, W, seed=s + 1))
    w = rnd(cout, cin, 3, 3, seed=s + 2, scale=math.sqrt(2.0 / (9 * cin)))
    b = rnd(cout, seed=s + 3, scale=0.1)
    conv64 = F.conv2d(x.double(), w.double(), None, padding=pad)
    oh, ow = conv64.shape[2:]
    return dict(x=x, w=w, b=b, conv64=conv64, base=rnd(n, cout, oh, ow, seed=s + 4), mask=rnd(n, cout, oh, ow, seed=s + 5))


@functools.lru_cache(maxsize=None)
def bwd_case(cg, c, H, W, n, pad=1):
    """The backward-data pass that consumes a gradient of cg channels on an H x W plane and produces c channels (the filters of the layer
    c -> cg, its backward bank): the gradient as such (g, masked: half zeros), as the gradient of the 2x2-pooled map (gp + the
    activation the pool's decisions come from), the feature map F of the produced gradient with a planted block of zeros and -0.0, and a
    small symmetric D for the Gram term.  A launch with padding `pad` is conv_transpose2d(., w, padding = 2 - pad)."""
    s = 977 * cg + 13 * c + H + W
    w = rnd(cg, c, 3, 3, seed=s + 1, scale=math.sqrt(2.0 / (9 * c)))
    g = rnd(n, cg, H, W, seed=s + 2) * (rnd(n, cg, H, W, seed=s + 3) > 0)
    act = torch.relu(rnd(n, cg, H, W, seed=s + 4))
    act[:, :, :4, :4] = 0.0                                           # all-zero windows: bit 2 of their decision bytes
    gp = rnd(n, cg, H // 2, W // 2, seed=s + 5)
    a64 = act.double().requires_grad_(True)
    F.max_pool2d(a64, 2, 2).backward(gp.double())
    unpooled64 = (a64.grad * (act > 0)).detach()
    oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
    f = torch.relu(rnd(n, c, oh, ow, seed=s + 6))
    f[:, :, : min(3, oh), : min(9, ow)] = 0.0
    f.view(n, c, -1)[:, 0::3, -1] = -0.0
    d = rnd(c, c, seed=s + 7) * 1e-3
    d = (d + d.t()).contiguous()
    tr = lambda t: F.conv_transpose2d(t, w.double(), padding=2 - pad)
    return dict(w=w, g=g, act=act, gp=gp, f=f, d=d, conv_g64=tr(g.double()), conv_unpooled64=tr(unpooled64),
                gram64=torch.einsum("kc,bkhw->bchw", d.double(), f.double()) if pad == 1 else None)


def pool_codes_of(hip, act):
    n, c, H, W = act.shape
    codes = torch.empty(n, c, H // 2, W // 2, dtype=torch.uint8, device="cuda")
    hip.pool2x2_fwd_codes(dev(act), torch.empty(n, c, H // 2, W // 2, device="cuda"), codes)
    return codes


def dmat_banks(hip, d, n):
    dbank, dinv = hip.conv_x3w_dmat_bank(d.shape[0], "cuda", frames=n)
    for i in range(n):
        hip.conv_pack_dmat_x3w(dev(d), dbank[i], dinv[i:i + 1])
    return dbank, dinv


def check_pooled(name, pooled, codes, full64, bar):
    """max_pool2d(full64) to `bar`, and decision bytes that name a maximum of the fp64 window (tests/test_conv_x3w_gpu.py)."""
    ref = F.max_pool2d(full64, 2, 2)
    check(name, pooled, ref, bar)
    n, c, ph, pw = ref.shape
    codes = planar_codes(codes.cpu())
    assert int(codes.max()) <= 7
    clear_sign = ref.abs() > 1e-5
    assert torch.equal(((codes & 4) != 0)[clear_sign], (ref <= 0)[clear_sign])
    pos = (codes & 3).long()
    rows = torch.arange(ph)[:, None] * 2 + pos // 2
    cols = torch.arange(pw)[None, :] * 2 + pos % 2
    picked = full64[torch.arange(n)[:, None, None, None], torch.arange(c)[None, :, None, None], rows, cols]
    assert float((picked - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. cot_inner = 1: conv_x3w / conv_x3q deal (pixel tile, channel tile) out as slot / ntile, slot % ntile
# ------------------------------------------------------------------------------------------------------------------------------------
# cin, cout, H, W, n: three channel tiles on a plane ragged on both edges (3 x 3 tiles of 8 x 32: 9 tiles on 8 XCDs, two per XCD and empty
# slots), a batch; one channel tile and one pixel tile (fewer tiles than XCDs).  The forced split needs four 16-channel chunks: cin 64.
X3W_SHAPES = [(32, 192, 19, 70, 2), (64, 64, 8, 32, 1)]
X3W_SPLIT_SHAPES = [(64, 192, 19, 70, 2), (64, 64, 8, 32, 1)]
X3W_FORMS = ["fwd", "acc", "mask", "acc_mask", "relu_pool", "unpool", "unpool_mask", "gram", "split", "split_armed"]


def x3w_launch(hip, form, cin, cout, H, W, n):
    """One launch form of conv_x3w_launch (conv_x3w.hip:974-980) -> ({name: result}, [(name, fp64 reference, bar)])."""
    if form in ("fwd", "acc", "mask", "acc_mask", "relu_pool", "split", "split_armed"):
        cs = fwd_case(cin, cout, H, W, n)
        bank, _, wsc = hip.conv_pack_filters_x3w(dev(cs["w"]))
        x, b, conv64 = dev(cs["x"]), dev(cs["b"]), cs["conv64"]
        biased = conv64 + cs["b"].double()[None, :, None, None]
        keep = cs["mask"] > 0
        if form == "fwd":
            y = hip.conv3x3_x3w(x, bank, wsc, b, cout, 1, True, out=nans(n, cout, H, W), workspace=one_pass_ws())
            return {"y": y}, [("y", torch.relu(biased), BAR)]
        if form == "acc":
            y = hip.conv3x3_x3w(x, bank, wsc, None, cout, 1, False, out=dev(cs["base"].clone()), accumulate=True, workspace=one_pass_ws())
            return {"y": y}, [("y", conv64 + cs["base"].double(), BAR)]
        if form == "mask":
            y = hip.conv3x3_x3w(x, bank, wsc, None, cout, 1, False, out=nans(n, cout, H, W), out_relu_mask=dev(cs["mask"]), workspace=one_pass_ws())
            return {"y": y}, [("y", conv64 * keep, BAR)]
        if form == "acc_mask":
            y = hip.conv3x3_x3w(x, bank, wsc, b, cout, 1, True, out=dev(cs["base"].clone()), out_relu_mask=dev(cs["mask"]), accumulate=True,
                                workspace=one_pass_ws())
            return {"y": y}, [("y", torch.relu(biased + cs["base"].double()) * keep, BAR)]
        if form == "relu_pool":
            pooled = nans(n, cout, H // 2, W // 2)
            codes = torch.full((n, cout, H // 2, W // 2), 255, dtype=torch.uint8, device="cuda")
            hip.conv3x3_x3w_relu_pool(x, bank, wsc, b, cout, 1, pooled, codes)
            return {"pooled": pooled, "codes": codes}, [("pool", torch.relu(biased), BAR)]
        # a channel loop split two ways: slabs + the finishing launch, or (armed) the last arriver of a tile adds them inside the launch
        assert hip.conv_x3w_split(n, cin, H, W, cout, 1) == 2
        ws = poisoned_ws(hip.conv_x3w_workspace_bytes(n, cin, H, W, cout, 1))
        hip.conv_arm_workspace(ws if form == "split_armed" else None)
        y = hip.conv3x3_x3w(x, bank, wsc, b, cout, 1, True, out=nans(n, cout, H, W), workspace=ws)
        ym = hip.conv3x3_x3w(x, bank, wsc, None, cout, 1, False, out=dev(cs["base"].clone()), out_relu_mask=dev(cs["mask"]), accumulate=True, workspace=ws)
        torch.cuda.synchronize()
        hip.conv_arm_workspace(None)
        return {"y": y, "ym": ym}, [("y", torch.relu(biased), BAR), ("ym", (conv64 + cs["base"].double()) * keep, BAR)]
    cs = bwd_case(cin, cout, H, W, n)
    _, bank, wsc = hip.conv_pack_filters_x3w(dev(cs["w"]))
    keep = cs["f"] > 0
    if form in ("unpool", "unpool_mask"):
        mask = dev(cs["f"]) if form == "unpool_mask" else None
        y = hip.conv3x3_x3w_unpool(dev(cs["gp"]), pool_codes_of(hip, cs["act"]), True, bank, wsc, cout, 1, out=nans(n, cout, H, W), out_relu_mask=mask,
                                   workspace=one_pass_ws())
        return {"y": y}, [("y", cs["conv_unpooled64"] * keep if mask is not None else cs["conv_unpooled64"], BAR)]
    assert form == "gram"
    dbank, dinv = dmat_banks(hip, cs["d"], n)
    y = hip.conv3x3_x3w_gram(dev(cs["g"]), bank, wsc, dev(cs["f"]), dbank, dinv, cout, 1, out=nans(n, cout, H, W), workspace=one_pass_ws())
    zbank, zinv = dmat_banks(hip, torch.zeros_like(cs["d"]), n)
    yc = hip.conv3x3_x3w_gram(dev(cs["g"]), bank, wsc, dev(cs["f"]), zbank, zinv, cout, 1, out=nans(n, cout, H, W), workspace=one_pass_ws())
    yg = hip.conv3x3_x3w_gram(dev(torch.zeros_like(cs["g"])), bank, wsc, dev(cs["f"]), dbank, dinv, cout, 1, out=nans(n, cout, H, W), workspace=one_pass_ws())
    # 3e-7 for the sum, BAR for each term alone: tests/test_x3w_gram_mask_gpu.py
    return {"y": y, "yc": yc, "yg": yg}, [("y", (cs["conv_g64"] + cs["gram64"]) * keep, 3e-7), ("yc", cs["conv_g64"] * keep, BAR), ("yg", cs["gram64"] * keep, BAR)]


def check_launch(out, refs):
    for name, ref64, bar in refs:
        if name == "pool":
            check_pooled(name, out["pooled"], out["codes"], ref64, bar)
        else:
            check(name, out[name], ref64, bar)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("form", X3W_FORMS)
def test_x3w_channel_tiles_side_by_side(hip, form, which):
    """cot_inner = 1 on every launch form of conv_x3w_launch: each result within the form's bar of fp64 and the bits of cot_inner = 0 (the
    mapping only says which workgroup computes a tile: conv_x3w.hip:223-229; a wrong one leaves tiles unwritten - NaN - or written twice
    from the wrong channel tile)."""
    split = form.startswith("split")
    cin, cout, H, W, n = (X3W_SPLIT_SHAPES if split else X3W_SHAPES)[which]
    assert (-(-H // 8) * -(-W // 32) > 8) == (which == 0)                 # (XW_ROWS = 8) more than one pixel tile per XCD
    ks = dict(x3w_ks=2) if split else {}
    force(hip, cot_inner=0, **ks)
    want, _ = x3w_launch(hip, form, cin, cout, H, W, n)
    force(hip, cot_inner=1, **ks)
    got, refs = x3w_launch(hip, form, cin, cout, H, W, n)
    torch.cuda.synchronize()
    check_launch(got, refs)
    same_bits(got, want)


# XQ_ROWS = 16: 35 x 70 is 3 x 3 = 9 pixel tiles (two per XCD and empty slots: with one tile per XCD slot / ntile is 0 and the mapping the
# identity), three channel tiles, a batch; and one tile, one channel tile
X3Q_SHAPES = [(256, 192, 35, 70, 2), (256, 64, 8, 32, 1)]
X3Q_FORMS = ["fwd", "bwd_mask", "relu_pool", "unpool", "unpool_mask", "split", "split_armed"]


@functools.lru_cache(maxsize=None)
def layer_bwd_ref(cin, cout, H, W, n, pad=1):
    """Backward-data of the layer of fwd_case: gy (masked by the layer's output) -> the input gradient in fp64, masked by the layer's input."""
    cs = fwd_case(cin, cout, H, W, n, pad)
    oh, ow = cs["conv64"].shape[2:]
    gy = rnd(n, cout, oh, ow, seed=5000 + cin + cout + H) * (torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None]) > 0)
    ref = torch.nn.grad.conv2d_input(cs["x"].shape, cs["w"].double(), gy.double(), padding=pad) * (cs["x"] > 0)
    return gy, ref


def x3q_launch(hip, form, cin, cout, H, W, n):
    if form in ("unpool", "unpool_mask"):
        cs = bwd_case(cin, cout, H, W, n)
        _, bank, wsc = hip.conv_pack_filters_x3q(dev(cs["w"]))
        mask = dev(cs["f"]) if form == "unpool_mask" else None
        y = hip.conv3x3_x3q_unpool(dev(cs["gp"]), pool_codes_of(hip, cs["act"]), True, bank, wsc, cout, 1, out=nans(n, cout, H, W), out_relu_mask=mask,
                                   workspace=one_pass_ws())
        return {"y": y}, [("y", cs["conv_unpooled64"] * (cs["f"] > 0) if mask is not None else cs["conv_unpooled64"], BAR)]
    cs = fwd_case(cin, cout, H, W, n)
    bank_f, bank_b, wsc = hip.conv_pack_filters_x3q(dev(cs["w"]))
    x, b = dev(cs["x"]), dev(cs["b"])
    act64 = torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None])
    if form == "fwd":
        y = hip.conv3x3_x3q(x, bank_f, wsc, b, cout, 1, True, out=nans(n, cout, H, W), workspace=one_pass_ws())
        return {"y": y}, [("y", act64, BAR)]
    if form == "bwd_mask":
        gy, ref = layer_bwd_ref(cin, cout, H, W, n)
        gx = hip.conv3x3_x3q(dev(gy), bank_b, wsc, None, cin, 1, False, out=nans(n, cin, H, W), out_relu_mask=x, workspace=one_pass_ws())
        return {"gx": gx}, [("gx", ref, BAR)]
    if form == "relu_pool":
        pooled = nans(n, cout, H // 2, W // 2)
        codes = torch.full((n, cout, H // 2, W // 2), 255, dtype=torch.uint8, device="cuda")
        hip.conv3x3_x3q_relu_pool(x, bank_f, wsc, b, cout, 1, pooled, codes)
        return {"pooled": pooled, "codes": codes}, [("pool", act64, BAR)]
    assert hip.conv_x3q_split(n, cin, H, W, cout, 1) == 2
    ws = poisoned_ws(hip.conv_x3q_workspace_bytes(n, cin, H, W, cout, 1))
    hip.conv_arm_workspace(ws if form == "split_armed" else None)
    y = hip.conv3x3_x3q(x, bank_f, wsc, b, cout, 1, True, out=nans(n, cout, H, W), workspace=ws)
    ym = hip.conv3x3_x3q(x, bank_f, wsc, None, cout, 1, False, out=dev(cs["base"].clone()), out_relu_mask=dev(cs["mask"]), accumulate=True, workspace=ws)
    torch.cuda.synchronize()
    hip.conv_arm_workspace(None)
    return {"y": y, "ym": ym}, [("y", act64, BAR), ("ym", (cs["conv64"] + cs["base"].double()) * (cs["mask"] > 0), BAR)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("form", X3Q_FORMS)
def test_x3q_channel_tiles_side_by_side(hip, form, which):
    """cot_inner = 1 on conv_x3q_launch's forms (conv_x3q.hip:853-859: plain, masked backward, pooling, unpooling with and without the
    mask, and a channel loop split two ways in both finishing forms): the form's bar against fp64, the bits of cot_inner = 0."""
    cin, cout, H, W, n = X3Q_SHAPES[which]
    assert (-(-H // 16) * -(-W // 32) > 8) == (which == 0)                # more than one pixel tile per XCD: slot / ntile is not always 0
    ks = dict(x3q_ks=2) if form.startswith("split") else {}
    force(hip, cot_inner=0, **ks)
    want, _ = x3q_launch(hip, form, cin, cout, H, W, n)
    force(hip, cot_inner=1, **ks)
    got, refs = x3q_launch(hip, form, cin, cout, H, W, n)
    torch.cuda.synchronize()
    check_launch(got, refs)
    same_bits(got, want)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. x3p_order = 0 (the channel tile outermost in conv_x3p's work list), 4. x3p_groups
# ------------------------------------------------------------------------------------------------------------------------------------
# cin, cout, H, W, n, pad: one chunk per item and three channel tiles on a ragged plane, a batch; no padding; a channel loop the cost model
# splits (one pixel tile); a channel loop split 3 + 2 chunks by x3p_ks = 2 on 3 x 2 pixel tiles x 3 channel tiles x 2 images (every digit of
# the item index - split, tile column, tile row, channel tile, image - has more than one value: the carries of `advance` all run)
X3P_SHAPES = [(32, 192, 70, 97, 2, 1), (64, 192, 66, 65, 1, 0), (512, 128, 16, 16, 2, 1), (160, 192, 19, 70, 2, 1)]
X3P_FORCED_KS = {3: 2}
X3P_FORMS = ["fwd", "bwd_mask", "pool", "unpool", "unpool_mask", "gram", "unpool_gram"]


def x3p_launch(hip, form, cin, cout, H, W, n, pad):
    """One form of conv_x3p_launch (conv_x3p.hip:1044-1052), in whatever split the cost model (or x3p_ks) picks -> ({name: result},
    references); None where the form does not exist for the geometry (the Gram term needs an output plane of the input's size).  Every
    launch gets slabs of its own that start as NaN: an (item, split) no workgroup computes must not find an earlier launch's sums."""
    oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
    slabs = lambda ci, h, w, co, p: dict(workspace=poisoned_ws(hip.conv_x3p_workspace_bytes(n, ci, h, w, co, p)))
    if form in ("fwd", "bwd_mask", "pool"):
        cs = fwd_case(cin, cout, H, W, n, pad)
        bank_f, bank_b, wsc = hip.conv_pack_filters_x3q(dev(cs["w"]))
        x, b = dev(cs["x"]), dev(cs["b"])
        act64 = torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None])
        if form == "fwd":
            return {"y": hip.conv3x3_x3p(x, bank_f, wsc, b, cout, pad, True, out=nans(n, cout, oh, ow), **slabs(cin, H, W, cout, pad))}, [("y", act64, BAR)]
        if form == "pool":
            pooled = nans(n, cout, oh // 2, ow // 2)
            codes = torch.full((n, cout, oh // 2, ow // 2), 255, dtype=torch.uint8, device="cuda")
            hip.conv3x3_x3p(x, bank_f, wsc, b, cout, pad, True, out=pooled, pool_codes=codes, **slabs(cin, H, W, cout, pad))
            return {"pooled": pooled, "codes": codes}, [("pool", act64, BAR)]
        if hip.conv_x3p_supported(cout, oh, ow, cin, 2 - pad):          # the layer's backward-data pass, masked by the layer's input
            gy, ref = layer_bwd_ref(cin, cout, H, W, n, pad)
            return {"gx": hip.conv3x3_x3p(dev(gy), bank_b, wsc, None, cin, 2 - pad, False, out=nans(n, cin, H, W), out_relu_mask=x,
                                              **slabs(cout, oh, ow, cin, 2 - pad))}, [("gx", ref, BAR)]
        assert cin % 64                                                   # (whole 64-channel tiles of the produced gradient: the masked form forwards)
        y = hip.conv3x3_x3p(x, bank_f, wsc, None, cout, pad, False, out=nans(n, cout, oh, ow), out_relu_mask=dev(cs["mask"]), **slabs(cin, H, W, cout, pad))
        return {"y": y}, [("y", cs["conv64"] * (cs["mask"] > 0), BAR)]
    if "gram" in form and pad != 1:
        return None
    cs = bwd_case(cin, cout, H, W, n, pad)
    _, bank, wsc = hip.conv_pack_filters_x3q(dev(cs["w"]))
    keep = cs["f"] > 0
    gram = dict(zip(("dmat_bank", "dmat_inv_scale"), dmat_banks(hip, cs["d"], n))) if "gram" in form else {}
    gram64 = cs["gram64"] if gram else 0.0
    if form == "gram":
        y = hip.conv3x3_x3p(dev(cs["g"]), bank, wsc, None, cout, pad, False, out=nans(n, cout, oh, ow), out_relu_mask=dev(cs["f"]), **gram, **slabs(cin, H, W, cout, pad))
        return {"y": y}, [("y", (cs["conv_g64"] + gram64) * keep, BAR)]
    mask = dev(cs["f"]) if form != "unpool" else None
    y = hip.conv3x3_x3p(dev(cs["gp"]), bank, wsc, None, cout, pad, False, out=nans(n, cout, oh, ow), out_relu_mask=mask, in_codes=pool_codes_of(hip, cs["act"]),
                        honour_relu_bit=True, **gram, **slabs(cin, H, W, cout, pad))
    return {"y": y}, [("y", (cs["conv_unpooled64"] + gram64) * keep if mask is not None else cs["conv_unpooled64"], BAR)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("form", X3P_FORMS)
def test_x3p_channel_tile_outermost(hip, form, which):
    """x3p_order = 0 - the second derivation of the digits a workgroup advances its item by (conv_x3p.hip:1021-1040, 207-231) - with 8, 16
    and 256 workgroups (with 8 or 16 every workgroup advances many times): BAR against fp64, and the bits of x3p_order = 1 whatever the
    number of workgroups (an item's sums are formed by one workgroup in its own chunk order; a split list is added in slab order).  The
    last shape runs under x3p_ks = 2: 5 chunks as 3 + 2 on a plane of several tiles, so that `advance` carries out of the split digit."""
    cin, cout, H, W, n, pad = X3P_SHAPES[which]
    if which in X3P_FORCED_KS:
        force(hip, x3p_ks=X3P_FORCED_KS[which])
    assert (hip.conv_x3p_split(n, cin, H, W, cout, pad) > 1) == (which >= 2)
    force(hip, x3p_order=1)
    hip.conv_x3p_set_max_groups(256)
    launched = x3p_launch(hip, form, cin, cout, H, W, n, pad)
    if launched is None:
        assert form in ("gram", "unpool_gram") and pad == 0
        return
    want, refs = launched
    torch.cuda.synchronize()
    check_launch(want, refs)
    for order, groups in ((0, 8), (0, 16), (0, 256), (1, 8)):
        force(hip, x3p_order=order)
        hip.conv_x3p_set_max_groups(groups)
        got, _ = x3p_launch(hip, form, cin, cout, H, W, n, pad)
        torch.cuda.synchronize()
        print("order", order, "groups", groups)
        check_launch(got, refs)
        same_bits(got, want)


@pytest.mark.parametrize("which", [0, 2, 3])
def test_x3p_groups_through_the_tuning_constant(hip, which):
    """x3p_groups = 8 / 16 with the setter left at 0: the bits of maua_conv_x3p_set_max_groups(8) / (16); a value below 8 is 256
    (x3p_max_groups(), conv_x3p.hip:974-977).  Every result against fp64 as well."""
    cin, cout, H, W, n, pad = X3P_SHAPES[which]
    if which in X3P_FORCED_KS:
        force(hip, x3p_ks=X3P_FORCED_KS[which])
    results = {}
    for label, setter, field in (("set8", 8, None), ("set16", 16, None), ("set256", 256, None), ("field8", 0, 8), ("field16", 0, 16), ("field4", 0, 4)):
        plan.OVERRIDES.pop("x3p_groups", None)
        force(hip, **({"x3p_groups": field} if field is not None else {}))
        hip.conv_x3p_set_max_groups(setter)
        for form in ("fwd", "unpool_mask"):
            got, refs = x3p_launch(hip, form, cin, cout, H, W, n, pad)
            torch.cuda.synchronize()
            check_launch(got, refs)
            results[label, form] = got
    for form in ("fwd", "unpool_mask"):
        same_bits(results["field8", form], results["set8", form])
        same_bits(results["field16", form], results["set16", form])
        same_bits(results["field4", form], results["set256", form])


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. forced, ragged splits of the channel loop: x3p_ks = 2, 3, 4; five and seven chunks under x3w_ks / x3q_ks
# ------------------------------------------------------------------------------------------------------------------------------------
def forced_split(nchunks, forced, whole):
    """x3p_choose_split / x3q_choose_split / x3w_choose_split under a forced K split: at most half the chunks; conv_x3p brings the number
    down to the non-empty ranges of ceil(nchunks / ks) chunks (`whole`, conv_x3p.hip:946)."""
    ks = forced if forced <= nchunks // 2 else (nchunks // 2 if nchunks >= 4 else 1)
    if not whole:
        return ks
    cps = -(-nchunks // ks)
    return -(-nchunks // cps)


@pytest.mark.parametrize("cout,H,W,n", [(64, 16, 32, 1), (192, 16, 32, 1), (64, 19, 70, 2), (192, 19, 70, 2)])
@pytest.mark.parametrize("ks", [2, 3, 4])
@pytest.mark.parametrize("cin", [160, 224, 256])
def test_x3p_forced_ragged_splits(hip, cin, ks, cout, H, W, n):
    """x3p_ks on 5 chunks (2 -> 3 + 2), 7 chunks (3 -> 3 + 3 + 1; 2 -> 4 + 3) and 8 (3 -> 3 + 3 + 2): forward with bias + ReLU and, where
    conv_x3p takes the layer's backward pass (cin % 64 == 0), that pass with its mask - the split is what x3p_choose_split's whole()
    predicts, BAR against fp64, and the same bits with 8 workgroups walking the (item, split) list as with 256."""
    force(hip, x3p_ks=ks)
    want_ks = forced_split(cin // 32, ks, True)
    assert hip.conv_x3p_split(n, cin, H, W, cout, 1) == want_ks and want_ks > 1
    assert (cin, ks, want_ks) in {(160, 2, 2), (160, 3, 2), (160, 4, 2), (224, 2, 2), (224, 3, 3), (224, 4, 3), (256, 2, 2), (256, 3, 3), (256, 4, 4)}
    cs = fwd_case(cin, cout, H, W, n)
    bank_f, bank_b, wsc = hip.conv_pack_filters_x3q(dev(cs["w"]))
    x, b = dev(cs["x"]), dev(cs["b"])
    outs = []
    for groups in (256, 8):
        hip.conv_x3p_set_max_groups(groups)
        ws = poisoned_ws(hip.conv_x3p_workspace_bytes(n, cin, H, W, cout, 1))
        y = hip.conv3x3_x3p(x, bank_f, wsc, b, cout, 1, True, out=nans(n, cout, H, W), workspace=ws)
        torch.cuda.synchronize()
        check(f"fwd groups {groups}", y, torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None]), BAR)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    if hip.conv_x3p_supported(cout, H, W, cin, 1):
        assert cin == 256
        assert hip.conv_x3p_split(n, cout, H, W, cin, 1) == forced_split(cout // 32, ks, True)
        gy, ref = layer_bwd_ref(cin, cout, H, W, n)
        ws = poisoned_ws(hip.conv_x3p_workspace_bytes(n, cout, H, W, cin, 1))
        gx = hip.conv3x3_x3p(dev(gy), bank_b, wsc, None, cin, 1, False, out=nans(n, cin, H, W), out_relu_mask=x, workspace=ws)
        torch.cuda.synchronize()
        check("bwd", gx, ref, BAR)


@pytest.mark.parametrize("cout,H,W,n", [(64, 8, 32, 1), (192, 19, 70, 2)])
@pytest.mark.parametrize("ks", [2, 3])
@pytest.mark.parametrize("family,cin", [("x3w", 80), ("x3w", 112), ("x3q", 160), ("x3q", 224)])
def test_x3w_x3q_forced_ragged_splits(hip, family, cin, ks, cout, H, W, n):
    """Five and seven chunks under x3w_ks / x3q_ks (the existing forced-split tests use powers of two): the last split is shorter
    (conv_x3w.hip:502-504, conv_x3q.hip:488), in the two-launch form and with the last arriver finishing in the launch - BAR against fp64,
    and the same bits from both forms (tests/test_finish_in_launch_gpu.py's claim)."""
    force(hip, **{family + "_ks": ks})
    split = getattr(hip, f"conv_{family}_split")
    chunk = 16 if family == "x3w" else 32
    assert split(n, cin, H, W, cout, 1) == forced_split(cin // chunk, ks, False) == min(ks, cin // chunk // 2)
    cs = fwd_case(cin, cout, H, W, n)
    bank, _, wsc = getattr(hip, f"conv_pack_filters_{family}")(dev(cs["w"]))
    conv = getattr(hip, f"conv3x3_{family}")
    ref = torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None])
    outs = []
    for armed in (False, True):
        ws = poisoned_ws(getattr(hip, f"conv_{family}_workspace_bytes")(n, cin, H, W, cout, 1))
        hip.conv_arm_workspace(ws if armed else None)
        y = conv(dev(cs["x"]), bank, wsc, dev(cs["b"]), cout, 1, True, out=nans(n, cout, H, W), workspace=ws)
        ym = conv(dev(cs["x"]), bank, wsc, None, cout, 1, False, out=dev(cs["base"].clone()), out_relu_mask=dev(cs["mask"]), accumulate=True, workspace=ws)
        torch.cuda.synchronize()
        hip.conv_arm_workspace(None)
        check(f"armed {armed}", y, ref, BAR)
        check(f"armed {armed}, accumulate + mask", ym, (cs["conv64"] + cs["base"].double()) * (cs["mask"] > 0), BAR)
        outs.append((y, ym))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. x3w_stagger: the start delay of the workgroups in the odd slot of a CU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,H,W,n", [(16, 128, 160, 256, 2), (64, 64, 8, 32, 1)])
def test_x3w_stagger_changes_no_bit(hip, cin, cout, H, W, n):
    """x3w_stagger = 0 and 3 against 7: a delay (s_sleep before the chunk loop, conv_x3w.hip:525-530: workgroups in the odd slot of their
    CU among the first 512) changes no bit.  (16, 128, 160 x 256, 2 images) is 8 x 20 tiles x 2 channel tiles x 2 images = 640 workgroups,
    more than the 512 slots of one round; (64, 64, 8 x 32) is eight workgroups of which one has work."""
    tiles = -(-W // 32) * -(-H // 8)
    wgs = -(-tiles // 8) * 8 * -(-cout // 64) * n
    assert wgs > 512 if cin == 16 else wgs < 512
    cs = fwd_case(cin, cout, H, W, n)
    bank, _, wsc = hip.conv_pack_filters_x3w(dev(cs["w"]))
    ref = torch.relu(cs["conv64"] + cs["b"].double()[None, :, None, None])
    outs = {}
    for stagger in (7, 0, 3):
        force(hip, x3w_stagger=stagger)
        outs[stagger] = hip.conv3x3_x3w(dev(cs["x"]), bank, wsc, dev(cs["b"]), cout, 1, True, out=nans(n, cout, H, W), workspace=one_pass_ws())
        torch.cuda.synchronize()
        check(f"stagger {stagger}", outs[stagger], ref, BAR)
    assert torch.equal(outs[0], outs[7]) and torch.equal(outs[3], outs[7])


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. conv_few_out, few_out_ks4_below: the three kernels behind a 3x3 pass that produces <= 4 channels
# ------------------------------------------------------------------------------------------------------------------------------------
# direction, consumed channels, produced channels, H, W of the LAYER's input, pad of the layer: the few-output shapes of
# tests/test_kernels_gpu.py's CONV_CASES, a plane of 17 rows (16 + 1 against the plain form's 4 waves x 4 rows, 2 x 8 + 1 against the
# strips of the form that splits the channels four ways), and several strips x several 62-column tiles
FEW_OUT_CASES = [("bwd", 64, 3, 70, 200, 1), ("fwd", 64, 4, 21, 130, 1), ("fwd", 32, 1, 40, 64, 1), ("bwd", 32, 2, 19, 63, 0), ("fwd", 64, 3, 17, 70, 1),
                 ("bwd", 64, 3, 17, 70, 1), ("fwd", 64, 3, 130, 130, 1)]


@functools.lru_cache(maxsize=None)
def few_out_case(direction, cons, prod, H, W, pad):
    n = 2
    s = 31 * cons + prod + H + W
    if direction == "fwd":
        x = rnd(n, cons, H, W, seed=s + 1)
        m = rnd(n, cons, H, W, seed=s + 2)
        w = rnd(prod, cons, 3, 3, seed=s + 3, scale=math.sqrt(2.0 / (9 * cons)))
        b = rnd(prod, seed=s + 4, scale=0.1)
        ref = lambda masked: F.conv2d((x * (m > 0) if masked else x).double(), w.double(), b.double(), padding=pad)
        return dict(x=x, m=m, w=w, b=b, ref={k: ref(k) for k in (False, True)})
    w = rnd(cons, prod, 3, 3, seed=s + 3, scale=math.sqrt(2.0 / (9 * prod)))   # the layer prod -> cons; its backward pass produces `prod`
    oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
    gy = rnd(n, cons, oh, ow, seed=s + 1)
    y = rnd(n, cons, oh, ow, seed=s + 2)                                          # the layer's output: the mask of the arriving gradient
    ref = lambda masked: torch.nn.grad.conv2d_input((n, prod, H, W), w.double(), (gy * (y > 0) if masked else gy).double(), padding=pad)
    return dict(gy=gy, y=y, w=w, ref={k: ref(k) for k in (False, True)})


def few_out_run(hip, direction, cons, prod, H, W, pad, masked):
    cs = few_out_case(direction, cons, prod, H, W, pad)
    wf, wb = hip.conv_pack_filters(dev(cs["w"]))
    if direction == "fwd":
        oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
        return hip.conv2d_fwd(dev(cs["x"]), wf, dev(cs["b"]), 3, 1, pad, False, out=nans(2, prod, oh, ow), in_mask=dev(cs["m"]) if masked else None)
    return hip.conv2d_bwd_data(dev(cs["gy"]), dev(cs["y"]) if masked else None, wb, dev(cs["w"]), (2, prod, H, W), 3, 1, pad, out=nans(2, prod, H, W))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("direction,cons,prod,H,W,pad", FEW_OUT_CASES)
def test_few_output_channels_in_all_three_kernels(hip, direction, cons, prod, H, W, pad, masked):
    """few_out_ks4_below = 0: conv3x3_few_out's plain form (KS4 = false, conv_direct.hip:322-341; at the defaults every tested grid is below
    1024 workgroups and takes the form that splits the channels over the four waves); few_out_ks4_below = 1000000: that form, forced;
    conv_few_out = 0: the general MFMA kernel with 1 ... 4 output channels.  Each against fp64 at TOL (tests/test_kernels_gpu.py), with and
    without the mask on the consumed map, two images; the two vector-ALU forms agree to 2e-6 (the same fp32 products, quarter sums)."""
    ref = few_out_case(direction, cons, prod, H, W, pad)["ref"][masked]
    outs = {}
    for label, fields in (("plain", dict(few_out_ks4_below=0)), ("ks4", dict(few_out_ks4_below=1000000)), ("mfma", dict(conv_few_out=0))):
        for k in ("few_out_ks4_below", "conv_few_out"):
            plan.OVERRIDES.pop(k, None)
        force(hip, **fields)
        outs[label] = few_out_run(hip, direction, cons, prod, H, W, pad, masked)
        torch.cuda.synchronize()
        check(label, outs[label], ref, TOL)
    e = rel_l2(outs["plain"].cpu(), outs["ks4"].cpu().double())
    print(f"plain against ks4: {e:.3e}")
    assert e <= 2e-6


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. gram_x3 = 0: the fp32-MFMA Gram kernel, and the per-layer loop of maua_gram_partial_batch
# ------------------------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(3, 5), (64, 1000), (96, 900), (128, 77), (512, 4), (200, 4131)]


@functools.lru_cache(maxsize=None)
def gram_case(C, HW, center):
    f = torch.relu(rnd(1, C, HW, 1, seed=11 + C + HW)) + (0.5 if center else 0.0)
    ff = f.reshape(C, HW).double()
    fc = ff - ff.mean(1, keepdim=True) if center else ff
    scale = 1.0 / (C * HW)
    return f, ff.mean(1), (fc @ fc.t()) * scale, scale


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C,HW", GRAM_SHAPES)
def test_gram_fp32_kernel_forward(hip, C, HW, center):
    """gram_x3 = 0 through maua_gram_fwd and maua_gram_fwd_mse_ledger: gram_partial_kernel (gram.hip:1087) in 64 x 64 blocks whatever the
    shape, the Gram matrix within TOL of fp64 and exactly symmetric, row means to 1e-6 (tests/test_kernels_gpu.py::test_gram_fwd_bwd's
    bars); D = grad_scale (G - T) and the loss within what an error of TOL in G allows."""
    force(hip, gram_x3=0)
    assert hip.gram_block(C, HW) == 64 and hip.gram_block(512, 16384) == 64 and hip.gram_block(128, 4096) == 64
    f, mean64, ref, scale = gram_case(C, HW, center)
    gram, mean = hip.gram_fwd(dev(f), scale, center, out=nans(C, C), mean_out=nans(C) if center else None)
    torch.cuda.synchronize()
    check("gram", gram, ref, TOL)
    assert torch.equal(gram, gram.t())
    if center:
        check("mean", mean, mean64, 1e-6)
    target = (0.5 * ref + 0.1 * ref.abs().max() * rnd(C, C, seed=5).double()).float()
    target = (target + target.t()).contiguous() * 0.5
    ls, gs = 0.5 / (C * C), 3.0 / (C * C)
    led = hip.loss_ledger(1, 2, "cuda")
    g1, d1, m1 = nans(C, C), nans(C, C), nans(C)
    hip.gram_fwd_mse_ledger(dev(f), scale, center, g1, m1, dev(target), d1, ls, gs, led[0], 1)
    losses, total = torch.zeros(1, 2, device="cuda"), torch.zeros(1, device="cuda")
    hip.loss_ledger_sum(led, losses, total)
    torch.cuda.synchronize()
    assert torch.equal(g1, gram) and (not center or torch.equal(m1, mean))
    diff = ref - target.double()
    assert float((d1.cpu().double() - gs * diff).norm()) <= TOL * gs * float(ref.norm())
    assert torch.equal(d1, d1.t())
    want_loss = ls * float((diff * diff).sum())
    assert abs(float(losses[0, 1]) - want_loss) <= 2 * ls * float(diff.norm()) * TOL * float(ref.norm()) + 1e-6 * want_loss


@pytest.mark.parametrize("center", [False, True])
def test_gram_fp32_kernel_partial_batch(hip, center):
    """gram_x3 = 0 sends maua_gram_partial_batch through its per-layer loop (gram.hip:1175-1181): the workspaces of maua_gram_partial
    byte for byte, through the batched finishing launch the Gram / D / loss of maua_gram_fwd_mse_ledger, each Gram within TOL of fp64 -
    and ready slabs (the image layer's) are refused: the fp32 kernel has no fold for them."""
    force(hip, gram_x3=0)
    led_a, led_b = hip.loss_ledger(1, 8, "cuda"), hip.loss_ledger(1, 8, "cuda")
    layers, want, slabs = [], [], []
    for k, (C, HW) in enumerate(GRAM_SHAPES):
        f, _, ref, scale = gram_case(C, HW, center)
        fd = dev(f)
        t = dev(rnd(C, C, seed=500 + k) * 0.1)
        nbytes = hip.gram_workspace_bytes(C, HW)
        g0, d0, m0 = nans(C, C), nans(C, C), nans(C)
        hip.gram_fwd_mse_ledger(fd, scale, center, g0, m0, t, d0, 0.5 / (C * C), 3.0 / (C * C), led_a[0], k, workspace=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
        want.append((g0, d0, m0, ref))
        ws1 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        hip.gram_partial(fd, center, nans(C), ws1)
        slabs.append(ws1)
        layers.append(dict(workspace=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), gram=nans(C, C), target=t, dmat=nans(C, C), c=C, hw=HW, scale=scale,
                           loss_scale=0.5 / (C * C), grad_scale=3.0 / (C * C), ledger=led_b[0], slot=k, f=fd, mean=nans(C) if center else None))
    fin = hip.GramFinishBatch(layers)
    fin.run_partial()
    torch.cuda.synchronize()
    for ws1, l in zip(slabs, layers):
        assert torch.equal(ws1, l["workspace"])
    fin.run()
    la, ta = torch.zeros(8, device="cuda"), torch.zeros(1, device="cuda")
    lb, tb = torch.zeros(8, device="cuda"), torch.zeros(1, device="cuda")
    hip.loss_ledger_sum(led_a, la, ta)
    hip.loss_ledger_sum(led_b, lb, tb)
    torch.cuda.synchronize()
    for (g0, d0, m0, ref), l in zip(want, layers):
        assert torch.equal(g0, l["gram"]) and torch.equal(d0, l["dmat"])
        if center:
            assert torch.equal(m0, l["mean"])
        check(f"gram c {l['c']} hw {l['hw']}", l["gram"], ref, TOL)
    assert torch.equal(la, lb) and torch.equal(ta, tb) and float(ta) > 0
    ready = dict(layers[1], f=None, mean=None, slabs=3)                 # three ready slabs of a single-tile layer (C = 64)
    with pytest.raises(hip.HipError, match=r"rc=-2.*ready slabs need the fp16x3 kernels' fold"):   # MAUA_E_UNSUPPORTED, from gram.hip:1177
        hip.GramFinishBatch([ready]).run_partial()


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. gram_bwd_x3 = 0: gram_bwd_kernel<ACC, MASK> and, for shapes it does not take, center_bias_kernel + the 1x1 MFMA kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram_bwd_case(C, HW):
    f = torch.relu(rnd(C, HW, seed=3 + C + HW))
    f[: min(C // 2, 5), : min(HW // 2, 12)] = 0.0                       # a planted block of zeros
    f[C - 1, 0::3] = -0.0
    f[0, HW - 1] = -0.0
    assert int((f > 0).sum()) >= 4 and bool((f == 0).any())
    d = rnd(C, C, seed=4 + C)
    d = (d + d.t()).contiguous()
    base = rnd(C, HW, seed=5 + C)
    mean = f.double().mean(1).float()
    return f, d, base, mean


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C,HW", [(128, 4608), (20, 36), (96, 901), (30, 77), (3, 5)])
def test_gram_backward_fp32_routes(hip, C, HW, center):
    """gram_bwd_x3 = 0: the four instantiations of gram_bwd_kernel<ACC, MASK> at (128, 4608) and (20, 36) (c % 4 == 0 and hw % 4 == 0,
    gram.hip:1339-1351) and center_bias_kernel + conv_mfma_dispatch's 1x1 kernel at the ragged shapes, with and without row means:
    [F > 0] (D (F - mean) + previous) within TOL of fp64, within 2e-6 of the fp16x3 route
    (tests/test_kernels_gpu.py::test_gram_bwd_fp32_route_subprocess), exact zeros wherever F <= 0 (-0.0 and the planted block too)."""
    f, d, base, mean = gram_bwd_case(C, HW)
    fc = f.double() - mean.double()[:, None] if center else f.double()
    prod = d.double() @ fc
    fd, dd, md = dev(f), dev(d), dev(mean) if center else None
    for acc in (False, True):
        for masked in (False, True):
            outs = {}
            for x3 in (0, 1):
                force(hip, gram_bwd_x3=x3)
                gf = dev(base.clone()) if acc else nans(C, HW)
                outs[x3] = hip.gram_bwd(dd, fd, md, gf, acc, relu_mask=fd if masked else None)
            torch.cuda.synchronize()
            want = prod + base.double() if acc else prod
            if masked:
                want = want * (f > 0)
            check(f"accumulate {acc} masked {masked}", outs[0], want, TOL)
            e = rel_l2(outs[0].cpu(), outs[1].cpu().double())
            print(f"against the fp16x3 route: {e:.3e}")
            assert e <= 2e-6
            if masked:
                assert bool((outs[0].cpu()[~(f > 0)] == 0).all()) and bool((outs[0].cpu()[f > 0] != 0).any())


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. gram_t128_min_hw = 64: 128 x 128 Gram blocks on maps of one, two (ragged) and fifteen 64-pixel stages
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 200, 256])
@pytest.mark.parametrize("mode", [2, 1])
def test_gram_128_blocks_on_short_maps(hip, mode, C):
    """gram_t128_min_hw = 64 with gram_t128 = 2 (ragged maps too) and 1 (whole stages): hip.gram_block says 128 where gram_tile128
    (gram.hip:992-997) does, and gram_x3_partial128_kernel runs slices of ONE stage, of a full and a 36-pixel stage, of 15 stages - at the
    default the blocks start at 16 stages.  Centred and not, within 2e-6 of fp64
    (tests/test_random_shapes_gpu.py::test_random_gram_shapes_against_fp64's bar for the fp16x3 kernels), exactly symmetric, the same
    bits on a second launch."""
    force(hip, gram_t128_min_hw=64, gram_t128=mode)
    for HW in (64, 100, 960):
        want128 = C >= 128 and HW >= 64 and (mode == 2 or HW % 64 == 0) and (C + 128) * HW < (1 << 29)
        assert want128 == (mode == 2 or HW != 100)
        assert hip.gram_block(C, HW) == (128 if want128 else 64)
        for center in (False, True):
            f = torch.relu(rnd(1, C, HW, 1, seed=C + HW))
            ff = f.reshape(C, HW).double()
            fc = ff - ff.mean(1, keepdim=True) if center else ff
            ref = fc @ fc.t() / (C * HW)
            gram, mean = hip.gram_fwd(dev(f), 1.0 / (C * HW), center, out=nans(C, C), mean_out=nans(C) if center else None)
            again, _ = hip.gram_fwd(dev(f), 1.0 / (C * HW), center, out=nans(C, C), mean_out=nans(C) if center else None)
            torch.cuda.synchronize()
            check(f"hw {HW} center {center}", gram, ref, 2e-6)
            assert torch.equal(gram, gram.t()) and torch.equal(gram, again)
            if center:
                check("mean", mean, ff.mean(1), 1e-6)


# ------------------------------------------------------------------------------------------------------------------------------------
# p1_order = 0: conv1x1_x3 in dispatch order (tests/test_kernels_gpu.py forces it for one forward launch per shape)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,H,W", [(100, 70, 9, 37), (96, 96, 40, 41), (512, 512, 32, 32)])
def test_conv1x1_in_dispatch_order(hip, cin, cout, H, W):
    """p1_order = 0 on the forward form (bias + ReLU), the masked and the accumulating backward form of conv1x1_x3 (the (512, 512, 32 x 32)
    case splits its channel loop): 2e-6 against fp64 (tests/test_kernels_gpu.py::test_conv1x1_x3_forward_and_backward) and the bits of
    p1_order = 1 (the order only says which workgroup computes an item: conv1x1_x3.hip:60-70, 322-326)."""
    x = rnd(2, cin, H, W, seed=1)
    w = rnd(cout, cin, seed=2, scale=math.sqrt(2.0 / cin))
    b = rnd(cout, seed=3, scale=0.1)
    gy = rnd(2, cout, H, W, seed=4)
    mask, base = rnd(2, cin, H, W, seed=6), rnd(2, cin, H, W, seed=5)
    ref = torch.relu(torch.einsum("oc,nchw->nohw", w.double(), x.double()) + b.double()[None, :, None, None])
    refb = torch.einsum("oc,nohw->nchw", w.double(), gy.double())
    wt = dev(w.t().contiguous())
    assert (hip.conv1x1_x3_workspace_bytes(2, cin, H * W, cout) > 0) == (cin == 512) == (hip.conv1x1_x3_workspace_bytes(2, cout, H * W, cin) > 0)
    slabs = lambda ci, co: dict(workspace=poisoned_ws(hip.conv1x1_x3_workspace_bytes(2, ci, H * W, co)))   # (NaN: of this launch alone)
    outs = {}
    for order in (1, 0):
        force(hip, p1_order=order)
        y = hip.conv1x1_x3(dev(x), dev(w), dev(b), relu=True, out=nans(2, cout, H, W), **slabs(cin, cout))
        gx = hip.conv1x1_x3(dev(gy), wt, out=nans(2, cin, H, W), out_relu_mask=dev(mask), **slabs(cout, cin))
        ga = hip.conv1x1_x3(dev(gy), wt, out=dev(base.clone()), accumulate=True, **slabs(cout, cin))
        torch.cuda.synchronize()
        check(f"order {order} forward", y, ref, 2e-6)
        check(f"order {order} masked", gx, refb * (mask > 0), 2e-6)
        check(f"order {order} accumulate", ga, refb + base.double(), 2e-6)
        outs[order] = {"y": y, "gx": gx, "ga": ga}
    same_bits(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# 10. L-BFGS: lbfgs_coeffs_kernel<4> (lbfgs_tri = 0), <8> (histories of 128 and more), the triangular kernel at its limit, the scalar sweeps
# ------------------------------------------------------------------------------------------------------------------------------------
def toy_problem(n, seed, sigma=0.1, cond=None):
    """tests/test_kernels_gpu.py::_toy_problem (a = 0.5 ... 3.5); with `cond`, its badly conditioned variant: a = 1 ... cond, log-uniform."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    a = u * 3 + 0.5 if cond is None else torch.exp(u * math.log(cond))
    q = 0.1 * n * n

    def fg(x):
        aa = a.to(x.device, x.dtype)
        r = torch.roll(x, 1)
        loss = sigma * ((aa * x * x).sum() + q * (x ** 4).sum() + 0.5 * (x * r).sum())
        grad = sigma * (2 * aa * x + 4 * q * x ** 3 + 0.5 * (r + torch.roll(x, -1)))
        return float(loss), grad
    return fg


@functools.lru_cache(maxsize=None)
def oracle_run(n, history, iters, cond=None):
    from oracle import lbfgs_run
    fg = toy_problem(n, seed=5, cond=cond)
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * (1.25 / n)  # |x0|_1 ~ 1
    x0 = x0.float().double()
    trace, stats = [], {}
    ref, _ = lbfgs_run(fg, x0, iters, history=history, trace=trace, stats=stats)
    return fg, x0, trace, stats, ref


def device_run_against_oracle(hip, n, history, iters):
    """The body of tests/test_kernels_gpu.py::test_lbfgs_matches_oracle: 2e-4 rel-L2 on the compared moves, final distance <= 1e-5 |x0|."""
    fg, x0, trace, stats, ref = oracle_run(n, history, iters)
    x = dev(x0.float())
    st = hip.LbfgsState(n, history, x.device)
    for it in range(iters):
        _, g = fg(x)
        st.iterate(x, g.contiguous())
        if it in (0, 1, 2, 3, 5, 8, 11):
            torch.cuda.synchronize()
            e = rel_l2(x.cpu(), trace[it])
            print(f"move {it}: {e:.3e}")
            assert e <= 2e-4, f"move {it}"
    torch.cuda.synchronize()
    s = st.status()
    # pairs with y.s <= 1e-10 are skipped by both (late, tiny steps); allow the borderline ones to differ
    assert s["n_iter"] == iters and abs(s["history_len"] - stats["history_len"]) <= 2 and not s["stopped"]
    assert s["history_len"] <= history
    dist = float((x.cpu().double() - ref).norm() / x0.norm())
    print(f"final distance / |x0|: {dist:.3e}")
    assert dist <= 1e-5
    return x


@pytest.mark.parametrize("n,history,iters", [(1000, 100, 30), (5000, 5, 40), (3 * 64 * 64 + 1, 100, 25), (40000, 7, 12), (1000, 126, 30), (1000, 127, 30)])
def test_lbfgs_recursion_kernel_without_the_triangular_form(hip, n, history, iters):
    """lbfgs_tri = 0: lbfgs_coeffs_kernel<4> (lbfgs.hip:865; the triangular kernel takes every history below 128 at the default), up to its
    limit - history 126: 255 coefficients, that of g at index 254, register 3 of lane 62 - and lbfgs_coeffs_kernel<8> from history 127
    (257 coefficients), which at the default starts at 128."""
    assert (2 * (history + 1) + 1 <= 256) == (history <= 126)
    force(hip, lbfgs_tri=0)
    device_run_against_oracle(hip, n, history, iters)


@pytest.mark.parametrize("history", [127, 128, 200, 254])
def test_lbfgs_long_histories(hip, history):
    """History 127: the triangular kernel at m1 = 128, its limit; 128, 200 and 254 (the largest the API accepts): lbfgs_coeffs_kernel<8>,
    whose coefficient of g sits in register 4 (history 128: index 258) ... 7 (history 254: index 510).  30 moves: the ring does not wrap."""
    device_run_against_oracle(hip, 1000, history, 30)


@pytest.mark.parametrize("n,history,iters", [(4096, 7, 12), (40000, 7, 12), (524288, 5, 6)])
def test_lbfgs_scalar_sweeps(hip, n, history, iters):
    """lbfgs_vec = 0 at counts that are multiples of four: lbfgs_pair_dots_kernel<false> and lbfgs_combine_kernel<1> (n < 524288) or <4>
    (n = 524288 = 256 x 4 x 512, lbfgs.hip:881).  Against the oracle only: the sums are NOT formed in the order of lbfgs_vec = 1 - a
    thread of the vector form holds elements 4 (tid + 256 j) ... + 3, a thread of the scalar form elements tid + 256 k
    (lbfgs.hip:178), so the per-thread partial sums of the dot products group other elements and the bits differ."""
    assert n % 4 == 0 and (n >= 256 * 4 * 512) == (n == 524288) and n < 256 * 16 * 512
    force(hip, lbfgs_vec=0)
    device_run_against_oracle(hip, n, history, iters)


@functools.lru_cache(maxsize=None)
def ring_problem():
    """The ring test's problem, the fp64 oracle's run, and the yardstick of a single move: the oracle's own recursion in fp32 arithmetic,
    TEACHER-FORCED (before every move its iterate is replaced by the fp64 run's, rounded to fp32) - the relative error of each of its
    moves x_k - x_(k-1) against the fp64 run's."""
    from oracle.style_oracle import _LbfgsState, _lbfgs_step
    n, history, iters = 3000, 128, 150
    fg, x0, trace, stats, _ = oracle_run(n, history, iters, cond=1e4)
    xs = [x0] + trace
    st, x, err32 = _LbfgsState(), x0.float(), []
    for it in range(iters):
        new = _lbfgs_step(x, lambda v: fg(v), st, 1, history)
        err32.append(rel_l2(new.double() - x.double(), xs[it + 1] - xs[it]))
        x = xs[it + 1].float()
    assert len(st.Y) == history
    return n, history, iters, fg, xs, stats, err32


def test_lbfgs_ring_wraps_in_the_recursion_kernel_with_eight_registers(hip):
    """History 128 over 150 moves of the badly conditioned problem (a = 1 ... 1e4, n = 3000), on which the fp64 oracle accepts a pair on every
    move: the ring of lbfgs_coeffs_kernel<8> fills (move 129) and wraps 21 times.

    TEACHER-FORCED: after every move the oracle's iterate, rounded to fp32, replaces the device vector, and every single MOVE
    x_k - x_(k-1) is compared with the oracle's (an iterate moves by 0.4 % ... 200 % of its length per move: a bar on the iterates would
    let a wrong direction pass).  A free run is not useful here: measured on the CPU, the oracle run in fp32 arithmetic from the same fp32
    x0 ends 2.2e-3 |x0| from the fp64 run (|x| has fallen to 5.6e-2 |x0| by then; at cond 1e3 ... 1e6 and sigma 0.1 ... 10: 2.1e-4 ... 7.1e-3,
    and at cond 1e3 only 98 of 149 pairs are accepted), so twice that plus the 1e-5 floor would allow an 8 % error of the final iterate.
    The bar of a move is the pattern of tests/test_engine_gpu.py's trajectories on single moves: twice the error of the oracle's own
    recursion in fp32, teacher-forced the same way (ring_problem: worst move measured: 2.3e-5 ... 2.8e-5 with the host's BLAS, a bar of 5.7e-5 ... 6.5e-5; the device's worst move: 2.9e-5 - both are
    set by the fp32 rounding of the iterates, 6e-8 |x| against moves of 4e-3 |x|), plus the 1e-5 floor; the first moves
    also meet the 2e-4 on the iterates of test_lbfgs_matches_oracle.  The device's pairs are s = t d of its own direction and
    y = g - g_prev of the gradients at the forced iterates: the oracle's pairs to fp32 rounding."""
    n, history, iters, fg, xs, stats, err32 = ring_problem()
    gs = [fg(x)[1] for x in xs[:-1]]
    ys = [float((gs[k] - gs[k - 1]).dot(xs[k] - xs[k - 1])) for k in range(1, len(gs))]
    assert len(xs) == iters + 1 and stats["history_len"] == history
    assert sum(v > 1e-10 for v in ys) == len(ys) == iters - 1 > history and min(ys) > 1e-9   # every pair accepted, none near the threshold (smallest: 6.0e-9)
    bar = 2 * max(err32) + 1e-5
    print(f"fp32 oracle, teacher-forced: worst move {max(err32):.3e} (move {err32.index(max(err32))}); bar {bar:.3e}")
    x = dev(xs[0].float())
    st = hip.LbfgsState(n, history, x.device)
    worst = 0.0
    for it in range(iters):
        prev = x.cpu().double()
        _, g = fg(x)
        st.iterate(x, g.contiguous())
        torch.cuda.synchronize()
        e = rel_l2(x.cpu().double() - prev, xs[it + 1] - xs[it])
        worst = max(worst, e)
        assert e <= bar, f"move {it}: {e:.3e}"
        if it in (0, 1, 2, 3, 5, 8, 11):
            assert rel_l2(x.cpu(), xs[it + 1]) <= 2e-4, f"iterate {it}"
        x.copy_(xs[it + 1].float())
    s = st.status()
    print(f"worst single move: {worst:.3e}")
    assert s["n_iter"] == iters and s["history_len"] == history and not s["stopped"]


# ------------------------------------------------------------------------------------------------------------------------------------
# 11. the routing thresholds of conv_x3q_preferred / conv_x3p_preferred
# ------------------------------------------------------------------------------------------------------------------------------------
def test_routing_thresholds(hip):
    """x3q_min_fill / x3q_min_chunks / x3p_min_fill / x3p_min_items: with thresholds of 0 every supported shape that runs in one pass is
    preferred, with one that cannot be met (a fill of 2.0, 10^9 chunks or items) none is; the defaults are back afterwards."""
    # n, cin, h, w, cout, pad
    q_shapes = [(2, 256, 35, 70, 192, 1), (1, 256, 8, 32, 64, 1), (1, 512, 64, 64, 512, 1)]
    p_shapes = [(2, 32, 70, 97, 192, 1), (1, 64, 66, 65, 192, 0), (1, 256, 256, 256, 256, 1)]   # (one pass each: conv_x3p_preferred asks for that first)
    before = [hip.conv_x3q_preferred(*s) for s in q_shapes] + [hip.conv_x3p_preferred(*s) for s in p_shapes]
    for s in p_shapes:
        assert hip.conv_x3p_supported(s[1], s[2], s[3], s[4], s[5]) and hip.conv_x3p_split(*s) == 1
    names = ("x3q_min_fill", "x3q_min_chunks", "x3p_min_fill", "x3p_min_items")
    zero = {k: 0 for k in names}
    force(hip, **zero)
    assert all(hip.conv_x3q_preferred(*s) for s in q_shapes) and all(hip.conv_x3p_preferred(*s) for s in p_shapes)
    for field, value in (("x3q_min_fill", 2.0), ("x3q_min_chunks", 10 ** 9)):
        force(hip, **dict(zero, **{field: value}))
        assert not any(hip.conv_x3q_preferred(*s) for s in q_shapes), field
        assert all(hip.conv_x3p_preferred(*s) for s in p_shapes)
    for field, value in (("x3p_min_fill", 2.0), ("x3p_min_items", 10 ** 9)):
        force(hip, **dict(zero, **{field: value}))
        assert not any(hip.conv_x3p_preferred(*s) for s in p_shapes), field
        assert all(hip.conv_x3q_preferred(*s) for s in q_shapes)
    for k in names:
        plan.OVERRIDES.pop(k, None)
    plan.forward_to_library(hip.lib())
    for k in names:
        assert hip.lib().maua_get_tuning(k.encode(), -1.0) == float(plan.FIELDS[k][0])
    assert before == [hip.conv_x3q_preferred(*s) for s in q_shapes] + [hip.conv_x3p_preferred(*s) for s in p_shapes]
