"""conv_x3w.hip's Gram-carrying launches take the ReLU mask of their epilogue from the Gram phase's own operand (tuning constant
`gram_mask_reuse`): a workgroup that runs the whole chunk list has already loaded every value of F its epilogue masks by, so it records
the bits F > 0 while the chunks of its channel tile are in registers, swaps them with lane ^ 32 (the same pixel column, the other channel
octet) and tests bits instead of loading F again.  Nothing in the arithmetic moves, so the bar is BIT IDENTITY with the loading epilogue
(`gram_mask_reuse` = 0), run after run, on F planted with everything the comparison can trip over: a block of exact zeros, -0.0, a positive
denormal, negative values, and - for EVERY channel, hence every residue mod 16 - a pixel where only that channel is positive (a bit taken
from the wrong lane, octet, chunk or register shows as a zero that should not be there and a value that should be zero).

Against fp64 the bars are the existing Gram tests' (tests/test_conv_x3w_gpu.py): 3e-7 rel-L2 for [F > 0] (conv_transpose(g) + D F), BAR for
the convolution and the Gram term alone.  "Clearly nonzero" in the pattern check means |fp64 value| > 1e-4 of the largest: the kernel's
element error is below 1e-5 of the largest value (the bound tests/test_conv_x3w_gpu.py asserts for picked elements), so such a value
cannot round to zero.

A split chunk list (`x3w_ks` = 2) must fall back to the loads - a split's workgroup sees only its own chunks of F - in the two-launch form
and when the last arriver finishes inside the launch.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import plan
from conftest import rel_l2
from test_conv_x3w_gpu import BAR, dev, hip, rnd  # noqa: F401  (hip: the module's fixture)

pytestmark = pytest.mark.gpu

GRAM_CASES = [(16, 64, 8, 32, 1), (32, 128, 16, 64, 2), (64, 80, 19, 45, 1), (64, 256, 24, 40, 1)]
UNPOOL_CASES = [(64, 64, 16, 64, 1), (32, 128, 18, 70, 2)]


@pytest.fixture(autouse=True)
def _restore(hip):
    yield
    for k in ("gram_mask_reuse", "x3w_ks"):
        plan.OVERRIDES.pop(k, None)
    plan.forward_to_library(hip.lib())
    hip.conv_arm_workspace(None)


def force(hip, **fields):
    for k, v in fields.items():
        plan.OVERRIDES[k] = str(v)
    plan.forward_to_library(hip.lib())


def planted_feature_map(n, c, H, W, seed):
    f = torch.relu(rnd(n, c, H, W, seed=seed))
    f[:, :, : min(4, H), : min(8, W)] = 0.0                     # a block of exact zeros
    flat = f.view(n, c, H * W)
    hw = H * W
    flat[:, 0::3, hw - 1] = -0.0
    flat[:, 1::3, hw - 1] = 1e-40                               # positive denormal: > 0
    flat[:, 2::3, hw - 1] = -1.5
    flat[:, 0::2, hw - 2] = 1e-40
    flat[:, 1::2, hw - 2] = -0.0
    stride = max(1, hw // (2 * c))                              # channel ch alone is positive at pixel 5 + ch * stride
    assert 5 + (c - 1) * stride < hw - 2
    neg = torch.tensor([0.0, -0.0, -2.0, -1e-40])
    for ch in range(c):
        px = 5 + ch * stride
        flat[:, :, px] = neg[(torch.arange(c) + ch) % 4]
        flat[:, ch, px] = 0.75 + 0.01 * ch
    assert bool((f == 0).any()) and bool((f < 0).any())
    return f


@functools.lru_cache(maxsize=None)
def case(kind, cin, c, H, W, n):
    """Inputs on the device and the fp64 references of one case, computed once."""
    s = 1000 * cin + c
    f = planted_feature_map(n, c, H, W, seed=s + 4)
    w = rnd(cin, c, 3, 3, seed=s + 3, scale=math.sqrt(2.0 / (9 * c)))
    d = rnd(c, c, seed=s + 5) * 1e-3
    d = (d + d.t()).contiguous()
    if kind == "gram":
        g = rnd(n, cin, H, W, seed=s + 1) * (rnd(n, cin, H, W, seed=s + 2) > 0)
        gfull, extra = g.double(), {"g": dev(g)}
    else:
        act = torch.relu(rnd(n, cin, H, W, seed=s + 1))
        act[:, :, :4, :4] = 0.0
        gp = rnd(n, cin, H // 2, W // 2, seed=s + 2)
        a64 = act.double().requires_grad_(True)
        F.max_pool2d(a64, 2, 2).backward(gp.double())
        gfull, extra = a64.grad * (act > 0), {"act": dev(act), "gp": dev(gp)}
    conv64 = F.conv_transpose2d(gfull, w.double(), padding=1)
    gram64 = torch.einsum("kc,bkhw->bchw", d.double(), f.double())
    return dict(extra, f=dev(f), keep=(f > 0), w=dev(w), d=dev(d), conv64=conv64, gram64=gram64)


def banks(hip, d, n):
    c = d.shape[0]
    dbank, dinv = hip.conv_x3w_dmat_bank(c, "cuda", frames=n)
    for i in range(n):
        hip.conv_pack_dmat_x3w(d, dbank[i], dinv[i:i + 1])
    return dbank, dinv


def check_against_fp64(out, ref64, keep, bar):
    out = out.cpu()
    ref = ref64 * keep
    print(f"rel_l2 {rel_l2(out, ref):.3e} (bar {bar:.1e})")
    assert rel_l2(out, ref) <= bar
    assert bool((out[~keep] == 0).all())                                   # exactly 0 wherever F <= 0 (-0.0 and the zeros included)
    clearly = keep & (ref64.abs() > 1e-4 * float(ref64.abs().max()))
    assert int(clearly.sum()) > 0 and bool((out[clearly] != 0).all())


def run_both_switches(hip, launch):
    """launch() with gram_mask_reuse 1, 1 again and 0: the three results must be the same bits."""
    force(hip, gram_mask_reuse=1)
    on, again = launch(), launch()
    force(hip, gram_mask_reuse=0)
    off = launch()
    force(hip, gram_mask_reuse=1)
    torch.cuda.synchronize()
    assert torch.equal(on, again)
    assert torch.equal(on, off)
    return on


@pytest.mark.parametrize("cin,c,H,W,n", GRAM_CASES)
def test_gram_backward_masks_from_its_own_operand(hip, cin, c, H, W, n):
    cs = case("gram", cin, c, H, W, n)
    _, bb, wsc = hip.conv_pack_filters_x3w(cs["w"])
    dbank, dinv = banks(hip, cs["d"], n)
    out = run_both_switches(hip, lambda: hip.conv3x3_x3w_gram(cs["g"], bb, wsc, cs["f"], dbank, dinv, c, 1))
    check_against_fp64(out, cs["conv64"] + cs["gram64"], cs["keep"], 3e-7)
    gram_only = run_both_switches(hip, lambda: hip.conv3x3_x3w_gram(torch.zeros_like(cs["g"]), bb, wsc, cs["f"], dbank, dinv, c, 1))
    check_against_fp64(gram_only, cs["gram64"], cs["keep"], BAR)
    zbank, zinv = banks(hip, torch.zeros_like(cs["d"]), n)
    conv_only = run_both_switches(hip, lambda: hip.conv3x3_x3w_gram(cs["g"], bb, wsc, cs["f"], zbank, zinv, c, 1))
    check_against_fp64(conv_only, cs["conv64"], cs["keep"], BAR)


def unpool_launches(hip, cs, cin, c, H, W, n, dbank, dinv, bb, wsc, gp=None):
    gp = cs["gp"] if gp is None else gp
    codes = torch.empty(n, cin, H // 2, W // 2, dtype=torch.uint8, device="cuda")
    hip.pool2x2_fwd_codes(cs["act"], torch.empty(n, cin, H // 2, W // 2, device="cuda"), codes)
    full = hip.pool2x2_bwd_codes(gp, codes, torch.empty(n, cin, H, W, device="cuda"), True)
    one = lambda: hip.conv3x3_x3w_unpool(gp, codes, True, bb, wsc, c, 1, out_relu_mask=cs["f"], dmat_bank=dbank, dmat_inv_scale=dinv)
    two = lambda: hip.conv3x3_x3w_gram(full, bb, wsc, cs["f"], dbank, dinv, c, 1)
    return one, two


@pytest.mark.parametrize("cin,c,H,W,n", UNPOOL_CASES)
def test_unpooling_gram_backward_masks_from_its_own_operand(hip, cin, c, H, W, n):
    cs = case("unpool", cin, c, H, W, n)
    _, bb, wsc = hip.conv_pack_filters_x3w(cs["w"])
    dbank, dinv = banks(hip, cs["d"], n)
    one, two = unpool_launches(hip, cs, cin, c, H, W, n, dbank, dinv, bb, wsc)
    out = run_both_switches(hip, one)
    assert torch.equal(out, run_both_switches(hip, two))                   # = pool2x2_bwd_codes + conv3x3_x3w_gram, bit for bit
    check_against_fp64(out, cs["conv64"] + cs["gram64"], cs["keep"], 3e-7)
    one_g, two_g = unpool_launches(hip, cs, cin, c, H, W, n, dbank, dinv, bb, wsc, gp=torch.zeros_like(cs["gp"]))
    gram_only = run_both_switches(hip, one_g)
    assert torch.equal(gram_only, run_both_switches(hip, two_g))
    check_against_fp64(gram_only, cs["gram64"], cs["keep"], BAR)
    zbank, zinv = banks(hip, torch.zeros_like(cs["d"]), n)
    one_c, two_c = unpool_launches(hip, cs, cin, c, H, W, n, zbank, zinv, bb, wsc)
    conv_only = run_both_switches(hip, one_c)
    assert torch.equal(conv_only, run_both_switches(hip, two_c))
    check_against_fp64(conv_only, cs["conv64"], cs["keep"], BAR)


@pytest.mark.parametrize("armed", [False, True])
def test_a_split_chunk_list_keeps_loading_the_mask(hip, armed):
    """x3w_ks = 2 on (64, 64, 16, 64, 1): every workgroup runs half of the chunk list, so none holds all the bits of its channel tile.  The
    launch must mask by loading F - in the finishing launch (not armed) and in the last arriver's epilogue (armed) - whatever the switch
    says: the same bits with the switch on and off, and the mask pattern and accuracy of the whole list."""
    cin, c, H, W, n = UNPOOL_CASES[0]
    cs = case("unpool", cin, c, H, W, n)
    _, bb, wsc = hip.conv_pack_filters_x3w(cs["w"])
    dbank, dinv = banks(hip, cs["d"], n)
    force(hip, x3w_ks=2)
    assert hip.conv_x3w_split(n, cin, H, W, c, 1) == 2
    ws = torch.full((hip.conv_x3w_workspace_bytes(n, cin, H, W, c, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    hip.conv_arm_workspace(ws if armed else None)
    gp, f = cs["gp"], cs["f"]
    codes = torch.empty(n, cin, H // 2, W // 2, dtype=torch.uint8, device="cuda")
    hip.pool2x2_fwd_codes(cs["act"], torch.empty(n, cin, H // 2, W // 2, device="cuda"), codes)
    full = hip.pool2x2_bwd_codes(gp, codes, torch.empty(n, cin, H, W, device="cuda"), True)
    out = run_both_switches(hip, lambda: hip.conv3x3_x3w_unpool(gp, codes, True, bb, wsc, c, 1, out_relu_mask=f, dmat_bank=dbank,
                                                                dmat_inv_scale=dinv, workspace=ws))
    two = run_both_switches(hip, lambda: hip.conv3x3_x3w_gram(full, bb, wsc, f, dbank, dinv, c, 1, workspace=ws))
    assert torch.equal(out, two)
    check_against_fp64(out, cs["conv64"] + cs["gram64"], cs["keep"], BAR)    # (the bar of the split-K forms in tests/test_conv_x3w_gpu.py)
