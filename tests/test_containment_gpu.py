"""Containment: no entry point of libmaua_hip writes outside its buffers, and no result depends on what lies beyond an input.

The other GPU modules hold values to fp64 references; none of them can see a store that lands a few elements or a whole tile behind an
output (torch's allocator pads and packs tensors), a workspace written past its `*_bytes()` promise, or a halo load whose out-of-range
value is multiplied by zero instead of being selected away.  Here every device argument of every case - inputs, outputs, workspaces,
banks, decision bytes, ledgers, states, counters - sits between guard bands (tests/guarded.py), workspaces / banks / ledgers / states at
exactly the byte count the matching `*_bytes()` query returns.  `TABLE` has one entry per case; a case names the C entry points it
exercises (tests/test_containment_table_cpu.py requires every entry point of include/maua_hip.h that takes a non-const pointer to be
named by some case).  Every case runs twice - input guards all 0x00, then all 0xFF (NaN as floats) - and after a synchronize:
  a. every guard of everything a kernel may write is intact (on failure: first / last changed byte relative to the payload's end);
  b. every defined element was written (outputs start as 0xFF bytes: floats finite, decision bytes <= 7), and where an entry point
     defines only part of a buffer the rest is bit-unchanged;
  c. the two runs' outputs and workspaces are bit-identical;
  d. one value check against the operation's fp64 reference at its existing bar (BAR / TOL of tests/test_tuning_variants_gpu.py, or the
     bar of the module named beside it) - a kernel that writes nothing does not pass.
Every new assertion is exact (pattern or bit equality); no new tolerance.

Shapes: the smallest at which each tiling can go wrong (a row and a column into a second tile, smaller than a tile, channels that are
no multiple of the tile or chunk, two images).  Where a family refuses a shape the nearest one it accepts stands in:
  - a forced split needs four chunks (conv_host.hpp choose_split): conv_x3w splits at cin 64, conv_x3q / conv_x3p at cin 128 (not 48 / 96);
  - the Gram form of conv_x3w needs cout % 16 == 0: 80 (not 72);
  - maua_conv_pack_dmat_x3w needs c % 16 == 0: 80 and 48 (not 70);
  - the conv_x3w / conv_x3q banks packed from 70 x 40 filters are consumed by launches with cin 48 / 64 (and 80 / 96 for the backward
    bank): the pack zero-fills the channels a chunk lacks, so the extra input channels must not count;
  - maua_conv_x3p_set_max_groups takes multiples of 8 (4 restores the default): 8 on the one-pass cases, 4 on the split ones;
  - maua_flow_consistency needs h, w >= 2: (2, 17) stands in for (1, 17);
  - maua_conv3x3_image_gram takes one image (it has no n): n = 1, not 2;
  - forms a family does not have are not run: conv_x3p takes no `accumulate`, conv_x3q has no Gram form, and conv_x3p has no in-launch
    finish, so its split cases are not armed (maua_conv_arm_workspace names the entry points it serves).

Which guards an argument gets: what an entry point only READS sits between the run's input guards (0x00, then 0xFF) - also where an
earlier call of the case produced it: the producer writes between 0xA5 guards that must stay intact, the consumer reads a copy between
input guards (filter and D banks, decision bytes, row means, statistics and coefficient tables, Gram slabs, the NCA partial slots, a
solver state, the L-BFGS state for maua_lbfgs_status).  Genuine in-out arguments keep one buffer between 0xA5 guards through all their
calls: ledgers (written by the *_ledger calls, emptied by the sum), the L-BFGS state and x through init / iterate, accumulate targets,
Adam's moments, split-K workspaces and their arrival counters.  A workspace that a split launch or a reduction must work in has to
change from its 0xFF bytes (`Ctx.used`): a wrapper that set it aside for a buffer of its own, or a launch that quietly ran one pass,
fails.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan
from conftest import rel_l2
from guarded import Guarded, PATTERN
from test_tuning_variants_gpu import BAR, TOL, _FORCED, bwd_case, check_pooled, force, fwd_case, oracle_run, rnd

pytestmark = pytest.mark.gpu

# entry point -> why it needs no case: the only admissible reason is that it writes no device memory
EXEMPT = {}

TABLE = []


class Case:
    def __init__(self, name, entries, fn, params):
        self.id = name + ("-" + "-".join(str(v) for v in params.values()) if params else "")
        self.entries, self.fn, self.params = tuple(entries), fn, params


def case(entries, params=(None,)):
    def deco(fn):
        for p in params:
            TABLE.append(Case(fn.__name__, entries(p) if callable(entries) else entries, fn, p or {}))
        return fn
    return deco


def declared_entry_points():
    return {e for c in TABLE for e in c.entries}


_INT = {1: torch.uint8, 4: torch.int32, 8: torch.int64}


def ibits(t):
    return t.view(_INT[t.element_size()])


class Ctx:
    """One run of one case: hands out guarded device arguments and remembers what has to hold afterwards."""

    def __init__(self, hip, fill):
        self.hip, self.L, self.fill = hip, hip.lib(), fill
        self.tracked, self.inputs, self.by_ptr, self.must_change = {}, [], {}, []

    def S(self):
        return self.hip._stream()

    def ok(self, rc, what):
        self.hip._check(rc, what)

    def inp(self, t):
        g = Guarded.of(t.contiguous(), guard_fill=self.fill)
        self.inputs.append(g)
        return g.payload

    def _track(self, name, g, kind):
        k, i = name, 1
        while k in self.tracked:
            i += 1
            k = f"{name}{i}"
        self.tracked[k] = dict(g=g, kind=kind, mask=None, before=None)
        self.by_ptr[g.ptr()] = k
        return g.payload

    def out(self, name, *shape, dtype=torch.float32, kind="float"):
        return self._track(name, Guarded(shape, dtype), kind)

    def codes(self, name, *shape):
        return self.out(name, *shape, dtype=torch.uint8, kind="codes")

    def inout(self, name, t, kind="float"):
        return self._track(name, Guarded.of(t.contiguous()), kind)

    def ws(self, name, nbytes):
        """A workspace / bank / state of EXACTLY nbytes (None for 0: the entry point is then handed no workspace)."""
        return self._track(name, Guarded((int(nbytes),), torch.uint8), "raw") if nbytes else None

    def used(self, payload):
        """A workspace the launch must really have worked in (its 0xFF bytes change): rules out a wrapper or an acceptance test that
        quietly sets the guarded workspace aside and runs one pass, or works in a buffer of its own."""
        if payload is not None:
            self.must_change.append(self.by_ptr[payload.data_ptr()])
        return payload

    def only(self, payload, pick):
        """The entry point defines only pick(payload); the rest of the payload must keep its bits."""
        rec = self.tracked[self.by_ptr[payload.data_ptr()]]
        mask = torch.zeros(payload.shape, dtype=torch.bool, device=payload.device)     # (in the shape the case views the payload in)
        pick(mask).fill_(True)
        rec["mask"], rec["before"] = mask.reshape(rec["g"].shape), rec["g"].payload.clone()

    def check(self, name, got, ref64, bar):
        e = rel_l2(got.detach().cpu(), ref64)
        print(f"  {name}: rel-L2 {e:.3e} (bar {bar:.1e})")
        assert e <= bar, f"{name}: rel-L2 {e:.3e} against fp64 (bar {bar:.1e})"

    def finish(self):
        torch.cuda.synchronize()
        bad, bits, sizes = [], {}, []
        for name, r in self.tracked.items():
            g, kind, mask = r["g"], r["kind"], r["mask"]
            sizes.append(f"{name} {g.nbytes} B")
            d = g.damage()
            if d:
                bad.append(f"{name}: guard overwritten, bytes {d['first']} .. {d['last']} relative to the end of its {d['payload_bytes']}-byte "
                           f"payload ({d['changed']} bytes changed)")
            p = g.payload
            defined = p[mask] if mask is not None else p
            if kind == "float" and not bool(torch.isfinite(defined).all()):
                bad.append(f"{name}: {int((~torch.isfinite(defined)).sum())} of {defined.numel()} defined elements were not written")
            if kind == "codes" and defined.numel() and int(defined.max()) > 7:
                bad.append(f"{name}: {int((defined > 7).sum())} of {defined.numel()} decision bytes were not written")
            if mask is not None and not torch.equal(ibits(p)[~mask], ibits(r["before"])[~mask]):
                bad.append(f"{name}: {int((ibits(p)[~mask] != ibits(r['before'])[~mask]).sum())} elements outside the defined part changed")
            bits[name] = g.bits()
        for name in self.must_change:
            if bool((self.tracked[name]["g"].payload_bytes == 0xFF).all()):
                bad.append(f"{name}: the workspace was handed over and never written")
        assert not bad, "; ".join(bad)
        return bits, sizes


def P(t):
    return t.data_ptr() if t is not None else None


def nb(t):
    return t.numel() * t.element_size() if t is not None else 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the tiled 3x3 families: conv_x3w, conv_x3q, conv_x3p
# ------------------------------------------------------------------------------------------------------------------------------------
N = 2
PACK_FAMILY = {"x3w": "x3w", "x3q": "x3q", "x3p": "x3q", "x3": "x3", "x6": "x6", "kxk_x3": "kxk_x3"}


def w_scale_of(w):
    return 2.0 ** (5 - math.floor(math.log2(float(w.abs().max()))))


def pack(c, fam, w, *ks):
    """Both banks of OIHW filters at exactly *_bank_bytes, packed through the C ABI between guards that must stay intact -> (forward bank,
    backward bank, w_scale), the banks as copies between the run's INPUT guards: that is what the convolutions read."""
    pf = PACK_FAMILY[fam]
    cout, cin = w.shape[:2]
    wsc = w_scale_of(w)
    bytes_of = getattr(c.L, f"maua_conv_{pf}_bank_bytes")
    bf, bb = c.ws("bank_fwd", bytes_of(cout, cin, *ks)), c.ws("bank_bwd", bytes_of(cin, cout, *ks))
    scale = () if pf == "x6" else (wsc,)
    c.ok(getattr(c.L, f"maua_conv_pack_filters_{pf}")(P(c.inp(w)), P(bf), P(bb), cout, cin, *ks, *scale, c.S()), f"maua_conv_pack_filters_{pf}")
    return c.inp(bf), c.inp(bb), wsc


def tiled_workspace(c, fam, cin, H, W, cout, pad, split, armed):
    need = getattr(c.L, f"maua_conv_{fam}_workspace_bytes")(N, cin, H, W, cout, pad)
    if split:
        assert getattr(c.L, f"maua_conv_{fam}_split")(N, cin, H, W, cout, pad) == 2 and need > 0
    ws = c.ws("workspace", need)
    if split:
        c.used(ws)
    if armed:
        c.hip.conv_arm_workspace(ws, counters=c.ws("counters", c.hip.ARRIVAL_COUNTER_BYTES), zero=True)
    return ws


def dmat_banks(c, d, n):
    nbytes = c.L.maua_conv_x3w_dmat_bank_bytes(d.shape[0])
    assert nbytes > 0
    bank, inv, dd = c.ws("dmat_bank", n * nbytes).view(n, nbytes), c.out("dmat_inv_scale", n), c.inp(d)
    for i in range(n):
        c.hip.conv_pack_dmat_x3w(dd, bank[i], inv[i:i + 1])
    return c.inp(bank), c.inp(inv)


def pool_codes(c, act):
    """The decision bytes of the 2x2 pool over `act` (odd planes: floor), produced between guards and handed on between input guards."""
    n, ch, H, W = act.shape
    y, codes = c.out("pool_y", n, ch, H // 2, W // 2), c.codes("pool_codes", n, ch, H // 2, W // 2)
    c.hip.pool2x2_fwd_codes(c.inp(act), y, codes)
    return c.inp(codes)


def tiled_entries(p):
    fam, form = p["fam"], p["form"]
    e = {"maua_conv_pack_filters_" + PACK_FAMILY[fam]}
    if fam == "x3p":
        e.add("maua_conv3x3_x3p")
    else:
        e.add("maua_conv3x3_" + fam + {"relu": "", "mask": "", "acc": "", "relu_pool": "_relu_pool", "unpool": "_unpool", "gram": "_gram"}[form])
    if form == "gram":
        e.add("maua_conv_pack_dmat_x3w")
    if p["armed"]:
        e.add("maua_conv_arm_workspace")
    return sorted(e)


def tiled_params(fam, cins, couts, planes, forms, split_cin, armed_too):
    out = []

    def add(cin, cout, H, W, pad, form, split, armed):
        oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
        if oh < 1 or ow < 1 or (form == "relu_pool" and (oh < 2 or ow < 2)) or (form == "gram" and pad != 1):
            return
        if form == "gram" and cout % 16:
            cout = 80
        out.append(dict(fam=fam, form=form, cin=cin, cout=cout, H=H, W=W, pad=pad, split=split, armed=armed))
    for cout in couts:
        for H, W in planes:
            for pad in (0, 1):
                for form in forms:
                    for cin in cins:
                        add(cin, cout, H, W, pad, form, 0, 0)
                    for armed in ((0, 1) if armed_too else (0,)):
                        add(split_cin, cout, H, W, pad, form, 1, armed)
    return out


TILED = (tiled_params("x3w", (16, 48), (72,), ((9, 33), (3, 5)), ("relu", "mask", "acc", "relu_pool", "unpool", "gram"), 64, True)
         + tiled_params("x3q", (32, 96), (72,), ((17, 33), (3, 5)), ("relu", "mask", "acc", "relu_pool", "unpool"), 128, True)
         + tiled_params("x3p", (32, 96), (64, 192), ((17, 33), (3, 5)), ("relu", "mask", "relu_pool", "unpool", "gram"), 128, False))


@case(tiled_entries, TILED)
def tiled_conv(c, fam, form, cin, cout, H, W, pad, split, armed):
    hip = c.hip
    if split:
        force(hip, **{fam + "_ks": 2})
    if fam == "x3p":
        assert hip.conv_x3p_supported(cin, H, W, cout, pad)
        hip.conv_x3p_set_max_groups(4 if split else 8)
    oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
    wrap = {"x3w": hip.conv3x3_x3w, "x3q": hip.conv3x3_x3q}.get(fam)
    if form in ("relu", "mask", "acc", "relu_pool"):
        cs = fwd_case(cin, cout, H, W, N, pad)
        bank, _, wsc = pack(c, fam, cs["w"])
        x, b = c.inp(cs["x"]), c.inp(cs["b"])
        biased = cs["conv64"] + cs["b"].double()[None, :, None, None]
        ws = tiled_workspace(c, fam, cin, H, W, cout, pad, split, armed)
        if form == "relu_pool":
            pooled, codes = c.out("pooled", N, cout, oh // 2, ow // 2), c.codes("codes", N, cout, oh // 2, ow // 2)
            if fam == "x3p":
                hip.conv3x3_x3p(x, bank, wsc, b, cout, pad, True, out=pooled, pool_codes=codes, workspace=ws)
            else:
                getattr(hip, f"conv3x3_{fam}_relu_pool")(x, bank, wsc, b, cout, pad, pooled, codes, workspace=ws)
            check_pooled("pool", pooled, codes, torch.relu(biased), BAR)
            return
        if form == "relu":
            y, kw, ref = c.out("y", N, cout, oh, ow), dict(bias=b, relu=True), torch.relu(biased)
        elif form == "mask":
            y, kw, ref = c.out("y", N, cout, oh, ow), dict(bias=None, relu=False, out_relu_mask=c.inp(cs["mask"])), cs["conv64"] * (cs["mask"] > 0)
        else:
            y, kw, ref = c.inout("y", cs["base"]), dict(bias=b, relu=False, accumulate=True), biased + cs["base"].double()
        if fam == "x3p":
            hip.conv3x3_x3p(x, bank, wsc, kw.pop("bias"), cout, pad, kw.pop("relu"), out=y, workspace=ws, **kw)
        else:
            wrap(x, bank, wsc, kw.pop("bias"), cout, pad, kw.pop("relu"), out=y, workspace=ws, **kw)
        c.check(form, y, ref, BAR)
        return
    cs = bwd_case(cin, cout, H, W, N, pad)
    _, bank, wsc = pack(c, fam, cs["w"])
    ws = tiled_workspace(c, fam, cin, H, W, cout, pad, split, armed)
    y = c.out("y", N, cout, oh, ow)
    if form == "unpool":
        # (a 9 x 33 or 17 x 33 plane is odd: its orphan row and column are staged as zeros)
        gp, codes = c.inp(cs["gp"]), pool_codes(c, cs["act"])
        if fam == "x3p":
            hip.conv3x3_x3p(gp, bank, wsc, None, cout, pad, False, out=y, in_codes=codes, honour_relu_bit=True, workspace=ws)
        else:
            getattr(hip, f"conv3x3_{fam}_unpool")(gp, codes, True, bank, wsc, cout, pad, out=y, workspace=ws)
        c.check("unpool", y, cs["conv_unpooled64"], BAR)
        return
    dbank, dinv = dmat_banks(c, cs["d"], N)
    g, f = c.inp(cs["g"]), c.inp(cs["f"])
    if fam == "x3p":
        hip.conv3x3_x3p(g, bank, wsc, None, cout, pad, False, out=y, out_relu_mask=f, dmat_bank=dbank, dmat_inv_scale=dinv, workspace=ws)
    else:
        hip.conv3x3_x3w_gram(g, bank, wsc, f, dbank, dinv, cout, pad, out=y, workspace=ws)
    c.check("gram", y, (cs["conv_g64"] + cs["gram64"]) * (cs["f"] > 0), 3e-7)     # tests/test_x3w_gram_mask_gpu.py: the bar of the sum


@case(lambda p: ("maua_conv_pack_filters_" + p["fam"], "maua_conv3x3_" + p["fam"]), [dict(fam="x3w"), dict(fam="x3q")])
def pack_ragged_tiled_banks(c, fam):
    """Banks from 70 x 40 filters (no multiple of the channel tile or the chunk), each consumed by a launch over the padded channels."""
    chunk = 16 if fam == "x3w" else 32
    wrap = getattr(c.hip, "conv3x3_" + fam)
    H, W = 9, 33
    w = rnd(70, 40, 3, 3, seed=901, scale=math.sqrt(2.0 / 360))
    bf, bb, wsc = pack(c, fam, w)
    up = lambda v: -(-v // chunk) * chunk
    x, g = rnd(N, up(40), H, W, seed=902), rnd(N, up(70), H, W, seed=903)
    y, gx = c.out("y", N, 70, H, W), c.out("gx", N, 40, H, W)
    wrap(c.inp(x), bf, wsc, None, 70, 1, False, out=y, workspace=c.ws("workspace", getattr(c.L, f"maua_conv_{fam}_workspace_bytes")(N, up(40), H, W, 70, 1)))
    wrap(c.inp(g), bb, wsc, None, 40, 1, False, out=gx, workspace=c.ws("workspace", getattr(c.L, f"maua_conv_{fam}_workspace_bytes")(N, up(70), H, W, 40, 1)))
    c.check("y", y, F.conv2d(x[:, :40].double(), w.double(), padding=1), BAR)
    c.check("gx", gx, F.conv_transpose2d(g[:, :70].double(), w.double(), padding=1), BAR)


@case(("maua_conv_pack_dmat_x3w", "maua_conv_pack_dmat_x3w_batch", "maua_conv3x3_x3w_gram"))
def pack_dmat(c):
    """The D banks of two layers (80 and 48 channels: no multiple of the 64-channel tile) by the per-layer call and by the batch call, each
    into frame 0 of a 2-frame (2, bytes) bank and a 2-frame scale - per-frame views as the engine hands them, frame 1 stays untouched;
    each bank consumed by a Gram-only launch (zero gradient)."""
    hip, items, runs = c.hip, [], []
    for ch in (80, 48):
        cs = bwd_case(16, ch, 9, 33, 1, 1)
        nbytes, d = c.L.maua_conv_x3w_dmat_bank_bytes(ch), c.inp(cs["d"])
        for how in ("single", "batch"):
            banks, invs = c.ws(f"dmat_banks_{ch}_{how}", 2 * nbytes).view(2, nbytes), c.out(f"inv_scales_{ch}_{how}", 2)
            c.only(banks, lambda m: m[0])
            c.only(invs, lambda m: m[0:1])
            if how == "single":
                hip.conv_pack_dmat_x3w(d, banks[0], invs[0:1])
            else:
                items.append((d, banks[0], invs[0:1]))
            runs.append((cs, ch, how, banks, invs))
    hip.DmatPackBatch(items).run()
    for cs, ch, how, banks, invs in runs:
        _, bank, wsc = pack(c, "x3w", cs["w"])
        y = c.out(f"y_{ch}_{how}", 1, ch, 9, 33)
        hip.conv3x3_x3w_gram(c.inp(torch.zeros_like(cs["g"])), bank, wsc, c.inp(cs["f"]), c.inp(banks[0]), c.inp(invs[0:1]), ch, 1, out=y, workspace=None)
        c.check(f"gram {ch} {how}", y, cs["gram64"] * (cs["f"] > 0), BAR)


# ------------------------------------------------------------------------------------------------------------------------------------
# conv_x3, conv_x6, conv_kxk_x3, conv1x1_x3, the fp32 / direct convolutions, the image layer and its backward pass
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer(cin, cout, H, W, k, stride=1, pad=None, n=N):
    pad = k // 2 if pad is None else pad
    s = 37 * cin + 5 * cout + H + W + k
    x = rnd(n, cin, H, W, seed=s + 1)
    w = rnd(cout, cin, k, k, seed=s + 2, scale=math.sqrt(2.0 / (k * k * cin)))
    b = rnd(cout, seed=s + 3, scale=0.1)
    y64 = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    gy = rnd(*y64.shape, seed=s + 4)
    gx64 = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), stride=stride, padding=pad)
    return dict(x=x, w=w, b=b, y64=y64, gy=gy, gx64=gx64, pad=pad, mask_y=rnd(*y64.shape, seed=s + 5), mask_x=rnd(n, cin, H, W, seed=s + 6))


@case(lambda p: ("maua_conv_pack_filters_" + p["fam"], {"kxk_x3": "maua_conv_kxk_x3"}.get(p["fam"], "maua_conv3x3_" + p["fam"])),
      [dict(fam=f, cin=ci) for f in ("x3", "x6", "kxk_x3") for ci in (40, 256)])
def dense_conv(c, fam, cin):
    """cin 40 -> cout 70 on 9 x 37, two images: forward (bias, ReLU) with the forward bank, backward-data (masked) with the backward bank;
    cin 256: the channel loop splits on a workspace of exactly *_workspace_bytes."""
    k = 5 if fam == "kxk_x3" else 3
    ks = (k,) if fam == "kxk_x3" else ()
    cout, H, W = 70, 9, 37
    cs = layer(cin, cout, H, W, k)
    bf, bb, wsc = pack(c, fam, cs["w"], *ks)
    need = getattr(c.L, f"maua_conv_{fam}_workspace_bytes")
    wrap = getattr(c.hip, "conv_kxk_x3" if fam == "kxk_x3" else "conv3x3_" + fam)
    scale = () if fam == "x6" else (wsc,)
    nf, nbk = need(N, cin, H, W, cout, *ks, k // 2), need(N, cout, H, W, cin, *ks, k // 2)
    assert (nf > 0) == (cin == 256)
    y, gx = c.out("y", N, cout, H, W), c.out("gx", N, cin, H, W)
    wrap(c.inp(cs["x"]), bf, *scale, c.inp(cs["b"]), cout, *ks, k // 2, True, out=y, workspace=c.used(c.ws("workspace", nf)))
    wrap(c.inp(cs["gy"]), bb, *scale, None, cin, *ks, k // 2, False, out=gx, out_relu_mask=c.inp(cs["mask_x"]), workspace=c.ws("workspace", nbk))
    c.check("y", y, torch.relu(cs["y64"]), BAR)
    c.check("gx", gx, cs["gx64"] * (cs["mask_x"] > 0), BAR)


@case(("maua_conv1x1_x3",), [dict(cin=40), dict(cin=256)])
def conv1x1(c, cin):
    cout, H, W = 70, 9, 37
    cs = layer(cin, cout, H, W, 1)
    shift = rnd(cin, seed=77, scale=0.3)
    need = c.L.maua_conv1x1_x3_workspace_bytes(N, cin, H * W, cout)
    assert (need > 0) == (cin == 256)
    y = c.out("y", N, cout, H, W)
    c.hip.conv1x1_x3(c.inp(cs["x"]), c.inp(cs["w"].reshape(cout, cin)), bias=c.inp(cs["b"]), relu=True, out=y, workspace=c.used(c.ws("workspace", need)),
                     x_shift=c.inp(shift))
    ref = torch.einsum("oc,nchw->nohw", cs["w"].reshape(cout, cin).double(), cs["x"].double() - shift.double()[None, :, None, None])
    c.check("y", y, torch.relu(ref + cs["b"].double()[None, :, None, None]), BAR)


@case(("maua_conv_pack_filters", "maua_conv2d_fwd", "maua_conv2d_bwd_data"),
      [dict(cin=3, cout=16, H=31, W=31, k=11, stride=4, pad=0), dict(cin=40, cout=24, H=9, W=31, k=1, stride=1, pad=0),
       dict(cin=40, cout=3, H=9, W=31, k=3, stride=1, pad=1), dict(cin=256, cout=24, H=9, W=31, k=1, stride=1, pad=0),
       dict(cin=40, cout=70, H=9, W=37, k=3, stride=1, pad=1)])
def conv2d(c, cin, cout, H, W, k, stride, pad):
    """The fp32 MFMA path (stride 1), the direct path (stride 4), the few-output route (cout 3) and a split channel loop (cin 256), with
    in_mask / out_mask / in_relu_mask; the filter banks of 70 x 40 (and the others) exactly cout * cin * k * k floats."""
    cs = layer(cin, cout, H, W, k, stride, pad)
    w = c.inp(cs["w"])
    wf, wb = c.out("wf", k * k, cin, cout), c.out("wb", k * k, cout, cin)
    c.ok(c.L.maua_conv_pack_filters(P(w), P(wf), P(wb), cout, cin, k, k, c.S()), "maua_conv_pack_filters")
    c.check("wf", wf, cs["w"].permute(2, 3, 1, 0).reshape(k * k, cin, cout).double(), TOL)
    c.check("wb", wb, cs["w"].flip(2, 3).permute(2, 3, 0, 1).reshape(k * k, cout, cin).double(), TOL)
    oh, ow = cs["y64"].shape[2:]
    nf = c.L.maua_conv_workspace_bytes(N, cin, H, W, cout, k, k, stride, pad)
    assert (nf > 0) == (cin == 256)
    y, gx = c.out("y", N, cout, oh, ow), c.out("gx", N, cin, H, W)
    wf_in, wb_in = c.inp(wf), c.inp(wb)                  # (what the convolutions read sits between the run's INPUT guards, like pack()'s banks)
    c.hip.conv2d_fwd(c.inp(cs["x"]), wf_in, c.inp(cs["b"]), k, stride, pad, True, out=y, in_mask=c.inp(cs["mask_x"]), workspace=c.used(c.ws("workspace", nf)))
    ref = F.conv2d(cs["x"].double() * (cs["mask_x"] > 0), cs["w"].double(), cs["b"].double(), stride=stride, padding=pad)
    c.check("y", y, torch.relu(ref), TOL)
    nbk = c.L.maua_conv_workspace_bytes(N, cout, oh, ow, cin, k, k, 1, k - 1 - pad) if stride == 1 else 0
    c.hip.conv2d_bwd_data(c.inp(cs["gy"]), c.inp(cs["mask_y"]), wb_in if stride == 1 else None, w if stride > 1 else None, (N, cin, H, W), k, stride, pad,
                          out=gx, in_relu_mask=c.inp(cs["mask_x"]), workspace=c.ws("workspace", nbk))
    ref = torch.nn.grad.conv2d_input(cs["x"].shape, cs["w"].double(), cs["gy"].double() * (cs["mask_y"] > 0), stride=stride, padding=pad)
    c.check("gx", gx, ref * (cs["mask_x"] > 0), TOL)


@case(("maua_conv_pack_filters_image", "maua_conv3x3_image"), [dict(cout=co, pad=p) for co in (24, 96) for p in (0, 2)])
def image_layer(c, cout, pad):
    """The canary of tests/test_conv_img_gpu.py (descriptor-masked stores of a 64-channel tile of which 24 exist) with two images, a plane
    of 33 x 31 and the paddings 0 and 2; the bank at exactly maua_conv_image_bank_bytes."""
    H, W = 33, 31
    cs = layer(3, cout, H, W, 3, 1, pad)
    bank = c.ws("bank", c.L.maua_conv_image_bank_bytes(cout, 3))
    c.ok(c.L.maua_conv_pack_filters_image(P(c.inp(cs["w"])), P(c.inp(cs["b"])), P(bank), cout, 3, c.S()), "maua_conv_pack_filters_image")
    y = c.out("y", *cs["y64"].shape)
    c.hip.conv3x3_image(c.inp(cs["x"]), c.inp(bank), cout, pad, True, out=y)
    c.check("y", y, torch.relu(cs["y64"]), BAR)         # tests/test_conv_img_gpu.py::test_image_layer_writes_nothing_outside_its_output: 2e-6


@case(("maua_conv_pack_filters_image", "maua_conv3x3_image_gram"), [dict(pad=0), dict(pad=2)])
def image_layer_gram(c, pad):
    H, W = 33, 31
    cs = layer(3, 64, H, W, 3, 1, pad, n=1)
    bank = c.ws("bank", c.L.maua_conv_image_bank_bytes(64, 3))
    c.ok(c.L.maua_conv_pack_filters_image(P(c.inp(cs["w"])), P(c.inp(cs["b"])), P(bank), 64, 3, c.S()), "maua_conv_pack_filters_image")
    nslab = c.hip.conv_image_gram_slabs(H, W, pad)
    assert nslab > 0
    y, slabs = c.out("y", *cs["y64"].shape), c.ws("gram_slabs", nslab * 64 * 64 * 4)
    c.hip.conv3x3_image_gram(c.inp(cs["x"]), c.inp(bank), pad, y, slabs)
    c.check("y", y, torch.relu(cs["y64"]), BAR)
    f = y.double().cpu().reshape(64, -1)                 # tests/test_conv_img_gpu.py::test_image_layer_with_the_gram_matrix_along: 3e-7
    upper = torch.ones(64, 64, dtype=torch.bool).triu()
    upper[32:, :32] = False
    c.check("gram", slabs.view(torch.float32).view(nslab, 64, 64).double().sum(0).cpu()[upper], (f @ f.t())[upper], 3e-7)


@case(("maua_conv_pack_filters_few_mfma", "maua_conv3x3_few_mfma"),
      [dict(H=h, W=w, cin=ci, tile=t) for h, w in ((5, 7), (15, 63), (9, 4)) for ci in (1, 2, 3) for t in (1, 2, 3)])
def few_mfma(c, H, W, cin, tile):
    cs = layer(cin, 64, H, W, 3)
    assert c.hip.conv_few_mfma_supported(N, cin, H, W, 64, 1)
    bank = c.ws("bank", c.L.maua_conv_few_mfma_bank_bytes())
    c.ok(c.L.maua_conv_pack_filters_few_mfma(P(c.inp(cs["w"])), P(bank), 64, cin, c.S()), "maua_conv_pack_filters_few_mfma")
    gx = c.out("gx", N, cin, H, W)
    c.hip.conv3x3_few_mfma(c.inp(cs["gy"]), c.inp(bank), cin, out=gx, tile=tile)
    c.check("gx", gx, cs["gx64"], BAR)


# ------------------------------------------------------------------------------------------------------------------------------------
# pointwise.hip
# ------------------------------------------------------------------------------------------------------------------------------------
COUNTS = [dict(count=1), dict(count=1025), dict(count=4 * 1024 + 3)]


@case(("maua_relu_fwd", "maua_relu_bwd", "maua_fill", "maua_axpy", "maua_adam_step"), COUNTS)
def elementwise(c, count):
    hip = c.hip
    x, gy, a = rnd(count, seed=1) + 0.1, rnd(count, seed=2), rnd(count, seed=3)
    xi = c.inout("relu_x", x)
    hip.relu_(xi)
    c.check("relu", xi, torch.relu(x.double()), TOL)
    gx = c.out("relu_gx", count)
    hip.relu_bwd(c.inp(gy), c.inp(torch.relu(x)), out=gx)
    c.check("relu_bwd", gx, gy.double() * (x > 0), TOL)
    filled = c.out("filled", count)
    hip.fill_(filled, 2.5)
    c.check("fill", filled, torch.full((count,), 2.5, dtype=torch.float64), TOL)
    y = c.inout("axpy_y", a)
    hip.axpy_(y, c.inp(x), -0.75)
    c.check("axpy", y, a.double() - 0.75 * x.double(), TOL)
    m0, v0 = rnd(count, seed=4) * 0.1, rnd(count, seed=5).abs() * 0.01
    px, pm, pv = c.inout("adam_x", x), c.inout("adam_m", m0), c.inout("adam_v", v0)
    hip.adam_step(px, c.inp(gy), pm, pv, 3, 0.1)
    m = 0.9 * m0.double() + 0.1 * gy.double()
    v = 0.999 * v0.double() + 0.001 * gy.double() ** 2
    c.check("adam m", pm, m, TOL)
    c.check("adam v", pv, v, TOL)
    c.check("adam x", px, x.double() - (0.1 / (1 - 0.9 ** 3)) * m / (v.sqrt() / math.sqrt(1 - 0.999 ** 3) + 1e-8), TOL)


@case(("maua_mse_fwd_bwd", "maua_mse_weighted_fwd_bwd"), [dict(count=k["count"], acc=a) for k in COUNTS for a in (0, 1)])
def mse(c, count, acc):
    hip = c.hip
    x, t, base = rnd(count, seed=11), rnd(count, seed=12), rnd(count, seed=13)
    grad = c.inout("grad", base) if acc else c.out("grad", count)
    loss = c.out("loss", 1)
    hip.mse_fwd_bwd(c.inp(x), c.inp(t), grad, 0.37, 1.7, bool(acc), loss, workspace=c.ws("workspace", c.L.maua_reduce_workspace_bytes(count)))
    d = x.double() - t.double()
    c.check("loss", loss, 0.37 * (d ** 2).sum().reshape(1), TOL)
    c.check("grad", grad, acc * base.double() + 1.7 * d, TOL)
    planes = 3
    xs, ts, bs = rnd(1, planes, 1, count, seed=14), rnd(1, planes, 1, count, seed=15), rnd(1, planes, 1, count, seed=16)
    for wplanes in (1, planes):
        w = rnd(wplanes, 1, count, seed=17 + wplanes).abs()
        grad = c.inout(f"wgrad{wplanes}", bs) if acc else c.out(f"wgrad{wplanes}", 1, planes, 1, count)
        loss = c.out(f"wloss{wplanes}", 1)
        hip.mse_weighted_fwd_bwd(c.inp(xs), c.inp(w), c.inp(ts), grad, 0.37, 1.7, bool(acc), loss,
                                 workspace=c.ws("workspace", c.L.maua_reduce_workspace_bytes(planes * count)))
        w64 = w.double().reshape(1, wplanes, 1, count)
        d = xs.double() * w64 - ts.double()
        c.check("weighted loss", loss, 0.37 * (d ** 2).sum().reshape(1), TOL)
        c.check("weighted grad", grad, acc * bs.double() + 1.7 * w64 * d, TOL)


def tv64(x, strength):
    xr = x.double().clone().requires_grad_(True)
    loss = strength * ((xr[:, :, 1:, :] - xr[:, :, :-1, :]).abs().sum() + (xr[:, :, :, 1:] - xr[:, :, :, :-1]).abs().sum())
    loss.backward()
    return loss.detach().reshape(1), xr.grad


@case(("maua_tv_fwd_bwd",), [dict(frames=1, H=1, W=9), dict(frames=2, H=17, W=5)])
def tv(c, frames, H, W):
    """Per-frame views buf[b:b + 1] of the batch's tensors, as the engine hands them over (engine.py): only frame 1 is defined."""
    x = rnd(frames, 3, H, W, seed=21)
    b = frames - 1
    xg, grad, losses = c.inp(x), c.out("grad", frames, 3, H, W), c.out("losses", frames)
    c.only(grad, lambda m: m[b:b + 1])
    c.only(losses, lambda m: m[b:b + 1])
    c.hip.tv_fwd_bwd(xg[b:b + 1], grad[b:b + 1], 0.02, False, losses[b:b + 1], workspace=c.ws("workspace", c.L.maua_reduce_workspace_bytes(3 * H * W)))
    loss64, g64 = tv64(x[b:b + 1], 0.02)
    c.check("loss", losses[b:b + 1], loss64, TOL)
    c.check("grad", grad[b:b + 1], g64, TOL)


@case(("maua_mse_fwd_bwd_ledger", "maua_tv_fwd_bwd_ledger", "maua_loss_ledger_sum", "maua_loss_ledger_sum_f64", "maua_sum_small"))
def ledgers(c):
    """Records (frame 1, slot 2) and (frame 1, slot 0) of ledgers of exactly maua_loss_ledger_bytes(2, 3); the sums into guarded losses / totals
    (an empty record's loss keeps its value), and maua_sum_small into total[b:b + 1]."""
    hip, frames, slots = c.hip, 2, 3
    x, t = rnd(1, 3, 17, 5, seed=31), rnd(1, 3, 17, 5, seed=32)
    nbytes = c.L.maua_loss_ledger_bytes(frames, slots)
    stride = nbytes // 8 // (frames * slots)
    assert stride * 8 * frames * slots == nbytes
    xg, tg = c.inp(x), c.inp(t)
    d = x.double() - t.double()
    mse64, (tv_loss64, tv_g64) = 0.25 * (d ** 2).sum().reshape(1), tv64(x, 0.02)
    # the MSE record, summed by maua_loss_ledger_sum
    led = c.inout("ledger_mse", torch.zeros(frames, slots, stride, dtype=torch.float64), kind="raw")
    c.only(led, lambda m: m[1, 2])
    grad = c.out("grad_mse", 1, 3, 17, 5)
    hip.mse_fwd_bwd_ledger(xg, tg, grad, 0.25, 1.5, False, led[1], 2)
    losses, totals = c.inout("losses", torch.zeros(frames, slots)), c.out("totals", frames)
    c.only(losses, lambda m: m[1, 2])
    hip.loss_ledger_sum(led, losses, totals)
    c.check("mse loss", losses[1, 2:3], mse64, TOL)
    c.check("mse grad", grad, 1.5 * d, TOL)
    c.check("totals", totals, torch.cat([torch.zeros(1, dtype=torch.float64), mse64]), TOL)
    # the TV record, summed by maua_loss_ledger_sum_f64
    led2 = c.inout("ledger_tv", torch.zeros(frames, slots, stride, dtype=torch.float64), kind="raw")
    c.only(led2, lambda m: m[1, 0])
    grad2 = c.out("grad_tv", 1, 3, 17, 5)
    hip.tv_fwd_bwd_ledger(xg, grad2, 0.02, False, led2[1], 0)
    losses2, totals2, f64 = c.inout("losses2", torch.zeros(frames, slots)), c.out("totals2", frames), c.out("losses_f64", frames, slots, dtype=torch.float64)
    c.only(losses2, lambda m: m[1, 0])
    c.only(f64, lambda m: m[1, 0])
    hip.loss_ledger_sum(led2, losses2, totals2, losses_f64=f64)
    c.check("tv loss", losses2[1, 0:1], tv_loss64, TOL)
    c.check("tv loss f64", f64[1, 0:1], tv_loss64, TOL)
    c.check("tv grad", grad2, tv_g64, TOL)
    # maua_sum_small into one frame's total
    vals = rnd(5, seed=33)
    total = c.out("total", frames)
    c.only(total, lambda m: m[1:2])
    hip.sum_small(c.inp(vals), total[1:2])
    c.check("sum_small", total[1:2], vals.double().sum().reshape(1), TOL)


@case(("maua_pool2d_fwd", "maua_pool2d_bwd"),
      [dict(H=8, W=10, k=2, s=2, ceil=0, mode="max"), dict(H=9, W=11, k=3, s=2, ceil=1, mode="max"), dict(H=10, W=11, k=3, s=3, ceil=0, mode="max"),
       dict(H=9, W=11, k=3, s=2, ceil=1, mode="avg"), dict(H=8, W=10, k=2, s=2, ceil=0, mode="avg")])
def pool2d(c, H, W, k, s, ceil, mode):
    x = rnd(N, 3, H, W, seed=41)
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, k, s, ceil_mode=bool(ceil)) if mode == "max" else F.avg_pool2d(x64, k, s, ceil_mode=bool(ceil), count_include_pad=False)
    gy = rnd(*y64.shape, seed=42)
    y64.backward(gy.double())
    xg = c.inp(x)
    y, gx = c.out("y", *y64.shape), c.out("gx", N, 3, H, W)
    c.hip.pool2d_fwd(xg, k, s, bool(ceil), mode, out=y)
    c.hip.pool2d_bwd(c.inp(gy), xg, k, s, bool(ceil), mode, out=gx)
    c.check("y", y, y64.detach(), TOL)
    c.check("gx", gx, x64.grad, TOL)


@case(("maua_pool2x2_fwd_codes", "maua_pool2x2_bwd_codes"), [dict(H=6, W=7), dict(H=7, W=6), dict(H=7, W=7), dict(H=6, W=8)])
def pool2x2_codes(c, H, W):
    """The float2 / float4 store paths on planes with an orphan column, an orphan row, both, neither: the backward pass writes the whole
    plane (orphans as zeros) and nothing behind it."""
    ch = 8
    assert c.hip.pool2x2_codes_supported(N, ch, H, W)
    x = torch.relu(rnd(N, ch, H, W, seed=43)) + 0.01 * torch.rand(N, ch, H, W, generator=torch.Generator().manual_seed(44))
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 2, 2)
    gy = rnd(*y64.shape, seed=45)
    y64.backward(gy.double())
    y, codes, gx = c.out("y", *y64.shape), c.codes("codes", *y64.shape), c.out("gx", N, ch, H, W)
    c.hip.pool2x2_fwd_codes(c.inp(x), y, codes)
    c.hip.pool2x2_bwd_codes(c.inp(gy), c.inp(codes), gx, False)
    c.check("y", y, y64.detach(), TOL)
    c.check("gx", gx, x64.grad, TOL)


@case(("maua_space_to_depth", "maua_depth_to_space"), [dict(acc=0), dict(acc=1)])
def regroup(c, acc):
    """r = 4 with sites beyond the plane: 3 x 3 sites cover 12 x 12 of a 9 x 10 plane (zeros beyond it); 2 x 2 sites cover 8 x 8 of a 9 x 10
    output (zeros, or the accumulated-into values, beyond them)."""
    r, ch, H, W = 4, 3, 9, 10
    x = rnd(N, ch, H, W, seed=51)
    out = c.out("s2d", N, r * r * ch, 3, 3)
    c.hip.space_to_depth(c.inp(x), r, out)
    xp = F.pad(x.double(), (0, 12 - W, 0, 12 - H)).reshape(N, ch, 3, r, 3, r)              # n, c, qy, ry, qx, rx
    c.check("s2d", out, xp.permute(0, 3, 5, 1, 2, 4).reshape(N, r * r * ch, 3, 3), TOL)
    z, base = rnd(N, r * r * ch, 2, 2, seed=52), rnd(N, ch, H, W, seed=53)
    back = c.inout("d2s", base) if acc else c.out("d2s", N, ch, H, W)
    c.hip.depth_to_space(c.inp(z), r, back, accumulate=bool(acc))
    full = z.double().reshape(N, r, r, ch, 2, 2).permute(0, 3, 4, 1, 5, 2).reshape(N, ch, 8, 8)  # n, c, qy, ry, qx, rx
    c.check("d2s", back, F.pad(full, (0, W - 8, 0, H - 8)) + acc * base.double(), TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# gram.hip
# ------------------------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(64, 77), (96, 4), (200, 1000)]


@functools.lru_cache(maxsize=None)
def gram_case(C, hw):
    f = torch.relu(rnd(C, hw, seed=61 + C))
    t = rnd(C, C, seed=62 + C) * 0.1
    t = (t + t.t()).contiguous()
    mean = f.double().mean(1)
    scale = 1.0 / (C * hw)
    g64 = {0: scale * f.double() @ f.double().t(), 1: scale * (f.double() - mean[:, None]) @ (f.double() - mean[:, None]).t()}
    d = rnd(C, C, seed=63 + C) * 1e-2
    return dict(f=f, t=t, mean64=mean, g64=g64, scale=scale, d=(d + d.t()).contiguous(), mask=rnd(C, hw, seed=64 + C))


@case(("maua_gram_fwd", "maua_gram_row_means", "maua_gram_bwd"),
      [dict(C=C, hw=hw, center=ce, x3=1) for C, hw in GRAM_SHAPES for ce in (0, 1)] + [dict(C=200, hw=1000, center=1, x3=0)])
def gram(c, C, hw, center, x3):
    hip = c.hip
    if not x3:
        force(hip, gram_x3=0, gram_bwd_x3=0)
    cs = gram_case(C, hw)
    need = c.L.maua_gram_workspace_bytes(C, hw)
    assert need >= 4 * C + 256                           # (hip.gram_bwd would set a smaller workspace aside for one of its own)
    f = c.inp(cs["f"])
    grams, mean = c.out("grams", 2, C, C), (c.out("mean", C) if center else None)     # (frame 1 of a 2-frame buffer, as the engine hands it over)
    c.only(grams, lambda m: m[1:2])
    hip.gram_fwd(f, cs["scale"], bool(center), out=grams[1], mean_out=mean, workspace=c.used(c.ws("workspace", need)))
    c.check("gram", grams[1], cs["g64"][center], TOL)
    means = c.out("row_means", C)
    hip.gram_row_means(f, means, c.used(c.ws("workspace", need)))
    c.check("row means", means, cs["mean64"], TOL)
    if center:
        c.check("mean", mean, cs["mean64"], TOL)
    gf = c.out("gf", C, hw)
    hip.gram_bwd(c.inp(cs["d"]), f, c.inp(means) if center else None, gf, False, workspace=c.ws("workspace", need), relu_mask=c.inp(cs["mask"]))
    fc = cs["f"].double() - (cs["mean64"][:, None] if center else 0.0)
    c.check("gram_bwd", gf, (cs["d"].double() @ fc) * (cs["mask"] > 0), TOL)


@case(lambda p: ("maua_gram_fwd_mse_ledger",) if p["how"] == "fused" else
      ("maua_gram_partial" if p["how"] == "partial" else "maua_gram_partial_batch", "maua_gram_finish_mse_batch"),
      [dict(C=C, hw=hw, center=ce, how=how) for C, hw in GRAM_SHAPES for ce in (0, 1) for how in ("fused", "partial", "batch")])
def gram_mse(c, C, hw, center, how):
    """Gram + MSE against the target + D, the loss left in record 1 of a two-record ledger: in one call, or as the partial launch (alone or
    batched) and the batched finishing launch; per-frame views of 2-frame gram / dmat buffers, as the engine hands them over."""
    hip = c.hip
    cs = gram_case(C, hw)
    assert hip.gram_mse_ledger_supported(C)
    ws = c.used(c.ws("workspace", c.L.maua_gram_workspace_bytes(C, hw)))
    f, t = c.inp(cs["f"]), c.inp(cs["t"])
    grams, dmats, mean = c.out("grams", 2, C, C), c.out("dmats", 2, C, C), (c.out("mean", C) if center else None)
    c.only(grams, lambda m: m[1:2])
    c.only(dmats, lambda m: m[1:2])
    nbytes = c.L.maua_loss_ledger_bytes(1, 2)
    led = c.inout("ledger", torch.zeros(1, 2, nbytes // 16, dtype=torch.float64), kind="raw")
    c.only(led, lambda m: m[0, 1])
    ls, gs = 0.5 / (C * C), 3.0 / (C * C)
    if how == "fused":
        hip.gram_fwd_mse_ledger(f, cs["scale"], bool(center), grams[1], mean, t, dmats[1], ls, gs, led[0], 1, workspace=ws)
    else:
        lay = dict(workspace=ws, gram=grams[1], target=t, dmat=dmats[1], c=C, hw=hw, scale=cs["scale"], loss_scale=ls, grad_scale=gs, ledger=led[0], slot=1,
                   f=f, mean=mean)
        if how == "partial":
            hip.gram_partial(f, bool(center), mean, ws)
        else:
            hip.GramFinishBatch([lay]).run_partial()
        hip.GramFinishBatch([dict(lay, workspace=c.inp(ws))]).run()    # the finishing launch only reads the slabs: a copy between input guards
    losses, totals = c.inout("losses", torch.zeros(1, 2)), c.out("totals", 1)
    c.only(losses, lambda m: m[0, 1])
    hip.loss_ledger_sum(led, losses, totals)
    diff = cs["g64"][center] - cs["t"].double()
    c.check("gram", grams[1], cs["g64"][center], TOL)
    c.check("dmat", dmats[1], gs * diff, TOL)
    c.check("loss", losses[0, 1:2], ls * (diff ** 2).sum().reshape(1), TOL)
    if center:
        c.check("mean", mean, cs["mean64"], TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# image.hip, warp.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def jittered64(x, noise, amp):
    """x + fp32(amp * noise) with the noise drawn in the (B, W, H, 3) view (image.hip: jittered_pixel), as planes (3 B, h w) in fp64."""
    j = x + (torch.tensor(amp, dtype=torch.float32) * noise).permute(0, 3, 2, 1)
    return j.reshape(-1, x.shape[2] * x.shape[3]).double()


def stats64(planes, B, j):
    v = planes[[k * B + j for k in range(3)]]
    return torch.cat([v.sum(1), torch.stack([(v[a] * v[b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])])


def sqrt_cov64(st, B, hw, eps):
    """image.hip: sqrt_cov - mean per true channel, covariance of the three reshaped rows + eps I, its symmetric square root."""
    mu = torch.zeros(3, dtype=torch.float64)
    for j in range(B):
        for k in range(3):
            mu[(k * B + j) % 3] += st[j, k]
    mu /= hw * B
    idx = ((3, 4, 5), (4, 6, 7), (5, 7, 8))
    a = torch.zeros(3, 3, dtype=torch.float64)
    for r1 in range(3):
        for r2 in range(3):
            for j in range(B):
                m1, m2 = mu[(r1 * B + j) % 3], mu[(r2 * B + j) % 3]
                a[r1, r2] += st[j, idx[r1][r2]] - m1 * st[j, r2] - m2 * st[j, r1] + hw * m1 * m2
    a = a / (hw * B) + eps * torch.eye(3, dtype=torch.float64)
    e, v = torch.linalg.eigh(a)
    return mu, v @ torch.diag(e.clamp_min(0).sqrt()) @ v.t()


@case(("maua_channel_stats", "maua_color_match_solve", "maua_color_match_apply"))
def color_match(c):
    """Two frames of 5 x 7: statistics of slot j into out[j] (workspace of exactly maua_channel_stats_workspace_bytes), the solve into row 1
    of a (3, 16) table, the map of slot 1 alone: planes k * 2 + 1 of the output, the others untouched."""
    hip, B, H, W, amp = c.hip, 2, 5, 7, 1e-3
    gen = torch.Generator().manual_seed(71)
    x = torch.rand(B, 3, H, W, generator=gen) * torch.tensor([200.0, 120.0, 60.0]).view(1, 3, 1, 1) - 90
    src = torch.rand(1, 3, 6, 4, generator=gen) * torch.tensor([90.0, 150.0, 110.0]).view(1, 3, 1, 1) - 50
    noise_t, noise_s = torch.randn(B, W, H, 3, generator=gen), torch.randn(1, 4, 6, 3, generator=gen)
    xg, ng = c.inp(x), c.inp(noise_t)
    st_t, st_s = c.out("stats_target", B, 9, dtype=torch.float64), c.out("stats_source", 1, 9, dtype=torch.float64)
    hip.channel_stats(xg, ng, amp, out=st_t, workspace=c.ws("workspace", c.L.maua_channel_stats_workspace_bytes(H, W)))
    hip.channel_stats(c.inp(src), c.inp(noise_s), amp, out=st_s, workspace=c.ws("workspace", c.L.maua_channel_stats_workspace_bytes(6, 4)))
    one = c.out("stats_slot_1", B, 9, dtype=torch.float64)
    c.only(one, lambda m: m[1])
    ws1 = c.ws("workspace", c.L.maua_channel_stats_workspace_bytes(H, W))
    c.ok(c.L.maua_channel_stats(P(xg), P(ng), amp, B, 1, H, W, P(one[1]), P(ws1), nb(ws1), c.S()), "maua_channel_stats")
    pt, ps = jittered64(x, noise_t, amp), jittered64(src, noise_s, amp)
    t64, s64 = torch.stack([stats64(pt, B, j) for j in range(B)]), stats64(ps, 1, 0)[None]
    c.check("stats target", st_t, t64, TOL)
    c.check("stats source", st_s, s64, TOL)
    c.check("stats slot 1", one[1], t64[1], TOL)
    table = c.inout("coef", torch.zeros(3, 16))
    table[:, 15] = 1.0                                   # (the rows the solve does not write: marked ok, as other sources' solves would)
    c.only(table, lambda m: m[1])
    hip.color_match_solve(c.inp(st_t), H * W, c.inp(st_s), 6 * 4, 1e-2, table[1])
    mu_t, q_t = sqrt_cov64(t64, B, H * W, 1e-2)
    mu_s, q_s = sqrt_cov64(s64, 1, 6 * 4, 1e-2)
    M = q_s @ torch.linalg.inv(q_t)
    c.check("coef", table[1], torch.cat([M.flatten(), mu_t, mu_s, torch.ones(1, dtype=torch.float64)]), TOL)
    out = c.out("out", B, 3, H, W)
    planes = [k * B + 1 for k in range(3)]
    c.only(out, lambda m: m.view(B * 3, H, W)[1::B])
    coefs = c.inp(table)
    c.ok(c.L.maua_color_match_apply(P(xg), P(ng), amp, P(coefs[1]), P(coefs), 3, 0.5, 0, B, 1, H, W, P(out), c.S()), "maua_color_match_apply")
    v = pt[planes]
    want = torch.stack([0.5 * (M[k] @ (v - torch.stack([mu_t[p % 3] for p in planes])[:, None]) + mu_s[planes[k] % 3]) for k in range(3)])
    c.check("apply", out.view(B * 3, H * W)[planes], want, TOL)


@case(("maua_resize_bilinear", "maua_deprocess_u8", "maua_mask_u8_resize"))
def image_helpers(c):
    x = rnd(2, 3, 7, 9, seed=81) * 100
    y = c.out("resized", 2, 3, 13, 5)
    c.ok(c.L.maua_resize_bilinear(P(c.inp(x)), P(y), 6, 7, 9, 13, 5, float(np.float32(7) / np.float32(13)), float(np.float32(9) / np.float32(5)), c.S()),
         "maua_resize_bilinear")
    c.check("resize", y, F.interpolate(x, (13, 5), mode="bilinear", align_corners=False), 1e-6)   # tests/test_kernels_gpu.py: 1e-6 against ATen's fp32 kernel
    from oracle import deprocess_u8
    import load
    img = rnd(1, 3, 5, 7, seed=82) * 120
    u8 = c.out("u8", 5, 7, 3, dtype=torch.uint8, kind="raw")
    m = load._MEAN_BGR
    c.ok(c.L.maua_deprocess_u8(P(c.inp(img.reshape(3, 5, 7))), P(u8), 5, 7, float(m[0]), float(m[1]), float(m[2]), c.S()), "maua_deprocess_u8")
    assert torch.equal(u8.cpu(), deprocess_u8(img.clone()))          # tests/test_kernels_gpu.py::test_deprocess_u8_is_bit_exact
    mask = torch.randint(0, 256, (7, 9, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(83))
    out = c.out("mask", 1, 3, 13, 5)
    c.ok(c.L.maua_mask_u8_resize(P(c.inp(mask)), P(out), 7, 9, 3, 13, 5, c.S()), "maua_mask_u8_resize")
    want = F.interpolate((mask.permute(2, 0, 1).float() / 255.0)[None], size=(13, 5), mode="bilinear", align_corners=False)
    assert float((out.cpu() - want).abs().max()) <= 4e-7    # tests/test_temporal_device_gpu.py::test_mask_against_the_reference_masks


@case(("maua_flow_warp_grid",), [dict(h=2, w=2, oh=5, ow=7), dict(h=45, w=130, oh=30, ow=64)])
def warp_grid(c, h, w, oh, ow):
    import os
    import tempfile
    import load
    from test_temporal_device_gpu import FP32_ULP, grid_f64
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 3, w), indexing="ij")
    flow = (np.stack([2.5 * np.sin(yy) * np.cos(xx), -1.5 * np.cos(yy)], axis=2) + rng.normal(size=(h, w, 2))).astype(np.float32)
    grid = c.out("grid", 1, oh, ow, 2)
    ws = c.ws("workspace", c.L.maua_flow_warp_grid_workspace_bytes(h, w))
    c.ok(c.L.maua_flow_warp_grid(P(c.inp(torch.from_numpy(flow))), P(grid), h, w, oh, ow, P(ws), nb(ws), c.S()), "maua_flow_warp_grid")
    ref = grid_f64(flow, (oh, ow))
    with tempfile.TemporaryDirectory() as d:             # the bar of tests/test_temporal_device_gpu.py::check_grid: twice the fp32 host code's own distance
        load.write_flow(flow, os.path.join(d, "f.flo"))
        theirs = load.flow_warp_map(os.path.join(d, "f.flo"), (oh, ow))
    c.check("grid", grid, ref, max(2 * rel_l2(theirs, ref), FP32_ULP))


@case(("maua_grid_sample_border",), [dict(blend=0), dict(blend=1)])
def grid_sample(c, blend):
    from test_temporal_device_gpu import FP32_ULP, sample_f64, seeded_grid
    n, ch, hw_in = 2, 3, (33, 65)
    hw_out = hw_in if blend else (13, 5)
    gen = torch.Generator().manual_seed(91)
    x = torch.randn(n, ch, *hw_in, generator=gen) * 60
    grid = seeded_grid(gen, n, hw_in, hw_out)
    y = c.out("y", n, ch, *hw_out)
    bl = torch.randn(n, ch, *hw_in, generator=gen) * 60
    init = c.out("init", n, ch, *hw_out) if blend else None
    c.ok(c.L.maua_grid_sample_border(P(c.inp(x)), P(c.inp(grid)), P(y), n, ch, *hw_in, *hw_out, P(c.inp(bl)) if blend else None, 0.3, P(init), c.S()),
         "maua_grid_sample_border")
    ref = sample_f64(x, grid)                            # the bars of tests/test_temporal_device_gpu.py::test_grid_sample_on_seeded_cases
    c.check("sampled", y, ref, 2 * rel_l2(F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False), ref))
    if blend:
        want = 0.7 * bl.double() + 0.3 * x.double()
        assert bool(((init.cpu().double() - want).abs() <= FP32_ULP * want.abs()).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# flow.hip
# ------------------------------------------------------------------------------------------------------------------------------------
FLOW_SHAPES = [dict(h=1, w=17), dict(h=2, w=3), dict(h=37, w=53)]


@case(("maua_flow_grey_u8", "maua_flow_pyr_down", "maua_flow_warp_prep", "maua_flow_tvl1_step", "maua_flow_tvl1_blocked", "maua_flow_median5",
       "maua_flow_upsample", "maua_flow_consistency"), FLOW_SHAPES)
def flow_kernels(c, h, w):
    import flow_restatement as R
    from test_flow_gpu import _rand, _state
    L, S = c.L, c.S()
    rgb = torch.from_numpy(np.random.default_rng(h * w).integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    grey = c.out("grey", h, w)
    c.ok(L.maua_flow_grey_u8(P(c.inp(rgb)), P(grey), h, w, S), "maua_flow_grey_u8")
    c.check("grey", grey, R.grey(rgb.numpy()), 2e-7)                # the bars of tests/test_flow_gpu.py, kernel by kernel
    img = _rand((h, w), 0, 255, h * w)
    down = c.out("down", (h + 1) // 2, (w + 1) // 2)
    c.ok(L.maua_flow_pyr_down(P(c.inp(img)), P(down), h, w, S), "maua_flow_pyr_down")
    c.check("pyr_down", down, R.pyr_down(img.double()), 1e-6)
    i0, i1, u = _rand((h, w), 0, 255, 1), _rand((h, w), 0, 255, 2), _rand((2, h, w), -4, 4, 3)
    fields = c.out("fields", 3, h, w)
    c.ok(L.maua_flow_warp_prep(P(c.inp(i0)), P(c.inp(i1)), P(c.inp(u)), P(fields), h, w, S), "maua_flow_warp_prep")
    want = R.warp_prep(i0.double(), i1.double(), u.double())
    for k in range(3):
        c.check(f"warp_prep {k}", fields[k], want[k], 1e-5)
    s, f = _state(h, w, 11)
    sg, fg = c.inp(s), c.inp(f)
    one, again, two = c.out("state_step", 6, h, w), c.out("state_step_2", 6, h, w), c.out("state_blocked", 6, h, w)
    c.ok(L.maua_flow_tvl1_step(P(fg), P(sg), P(one), h, w, S), "maua_flow_tvl1_step")
    c.ok(L.maua_flow_tvl1_step(P(fg), P(c.inp(one)), P(again), h, w, S), "maua_flow_tvl1_step")
    c.ok(L.maua_flow_tvl1_blocked(P(fg), P(sg), P(two), h, w, 2, S), "maua_flow_tvl1_blocked")
    want = R.tv_step(f.double(), s.double())
    for k in range(6):
        c.check(f"tvl1_step {k}", one[k], want[k], 1e-6)
    assert torch.equal(two, again)                                   # tests/test_flow_gpu.py: k blocked iterations = k single steps, bit for bit
    x = _rand((2, h, w), -5, 5, 7)
    med = c.out("median", 2, h, w)
    c.ok(L.maua_flow_median5(P(c.inp(x)), P(med), h, w, 2, S), "maua_flow_median5")
    assert torch.equal(med.cpu(), R.median5(x))                      # tests/test_flow_gpu.py: an exact selection
    H2, W2 = 2 * h - 1 if h > 1 else 2, 2 * w - 1
    up = c.out("upsampled", 2, H2, W2)
    c.ok(L.maua_flow_upsample(P(c.inp(x)), h, w, P(up), H2, W2, 2, 2.0, S), "maua_flow_upsample")
    c.check("upsample", up, R.upsample(x.double(), H2, W2, 2.0), 1e-5)
    hc = max(h, 2)                                                   # (maua_flow_consistency needs two rows)
    f1, f2 = round_trip_flows(hc, w)
    want = R.mask_bytes(f1, f2)
    assert (want == 0).any() and ((want == 255).any() or hc < 37)   # (reliable pixels are 0: nothing like the 0xFF the output starts as)
    planes = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    out = c.out("consistency", hc, w, dtype=torch.uint8, kind="raw")
    ws = c.ws("workspace", L.maua_flow_consistency_workspace_bytes(hc, w))
    c.ok(L.maua_flow_consistency(P(c.inp(planes(f1))), P(c.inp(planes(f2))), P(out), hc, w, P(ws), nb(ws), S), "maua_flow_consistency")
    assert np.array_equal(out.cpu().numpy(), want)   # tests/test_flow_gpu.py::test_mask_is_pixel_identical_to_the_reference


def round_trip_flows(h, w):
    """(flow1, flow2) as (h, w, 2): a gentle contraction towards the centre and its inverse - every pixel stays inside the frame, the round
    trip closes and no motion edge shows, so small frames are reliable throughout (a frame's last row and column are unreliable under any
    flow that does not point inwards); from 37 rows on a spoiled corner of flow2 makes the 41 x 41 windows around it unreliable."""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    cy, cx = (h - 1) / 2, (w - 1) / 2
    f1 = np.stack([-0.01 * (x - cx) / max(cx, 0.5), -0.01 * (y - cy) / max(cy, 0.5)], axis=2).astype(np.float32)
    f2 = -f1
    if h >= 37:
        f2[:2, :2] += 5.0
    return f1, f2


@functools.lru_cache(maxsize=None)
def tvl1_reference():
    import flow_restatement as R
    from test_flow_gpu import _frames
    img1, img2, _ = _frames(33, 70, "rotation_zoom")
    return img1, img2, R.estimate(img1, img2, max_levels=5, warps=2, iters=12, dtype=torch.float64)


@case(("maua_flow_tvl1",))
def flow_tvl1(c):
    h, w = 33, 70
    img1, img2, want = tvl1_reference()
    lv = c.hip.flow_levels(h, w, 5)
    ws = c.ws("workspace", c.L.maua_flow_tvl1_workspace_bytes(h, w, lv))
    out = c.out("flow", 2, h, w)
    c.hip.flow_tvl1(c.inp(torch.from_numpy(img1)), c.inp(torch.from_numpy(img2)), lv, 2, 12, 4, out=out, workspace=ws)
    c.check("flow", out, want, TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# lbfgs.hip, nca.hip
# ------------------------------------------------------------------------------------------------------------------------------------
@case(("maua_lbfgs_init", "maua_lbfgs_iterate", "maua_lbfgs_status"), [dict(count=1001), dict(count=1024)])
def lbfgs(c, count):
    """Three moves (first step, one pair, two pairs) on a state of exactly maua_lbfgs_state_bytes: a count that is no multiple of four and
    one that is (the float4 sweeps).  Bar: the 2e-4 per move of tests/test_kernels_gpu.py::test_lbfgs_matches_oracle."""
    history, moves = 3, 3
    fg, x0, trace, _, _ = oracle_run(count, history, moves + 1)
    nbytes = c.L.maua_lbfgs_state_bytes(count, history)
    state, x, out5 = c.ws("state", nbytes), c.inout("x", x0.float()), c.out("status", 5)
    c.ok(c.L.maua_lbfgs_init(P(state), nbytes, count, history, c.S()), "maua_lbfgs_init")
    for it in range(moves):
        _, g = fg(x)
        c.ok(c.L.maua_lbfgs_iterate(P(state), P(x), P(c.inp(g.float())), None, count, history, 1.0, -1.0, -1.0, c.S()), "maua_lbfgs_iterate")
        c.check(f"move {it}", x, trace[it], 2e-4)
    c.ok(c.L.maua_lbfgs_status(P(c.inp(state)), count, history, P(out5), c.S()), "maua_lbfgs_status")
    n_iter, _, stopped = out5.tolist()[:3]
    assert n_iter == moves and stopped == 0


@case(("maua_nca_step", "maua_nca_step_bwd", "maua_nca_grad_finish"),
      [dict(chn=12, hidden=96, n=1, h=1, w=1, mode="ones"), dict(chn=16, hidden=128, n=2, h=7, w=13, mode="given"),
       dict(chn=12, hidden=96, n=2, h=7, w=13, mode="rate_map")])
def nca(c, chn, hidden, n, h, w, mode):
    """The smallest geometry maua_nca_supported accepts (one pixel) and a ragged one (182 pixels: three 64-pixel tiles, the second spans
    both images); workspace and gradient of exactly maua_nca_bwd_workspace_bytes / maua_nca_param_count."""
    import nca_restatement as R
    hip = c.hip
    assert hip.nca_supported(n, chn, hidden, h, w)
    params = R.case_params(chn, hidden, 1)
    x, g = R.case_state(chn, n, h, w)
    x64 = x.astype(np.float64)
    g = g * ~R.near_tie(x64, params, chn, hidden)[:, None]              # (tests/test_nca_bwd_gpu.py: no gradient through a ReLU at a tie)
    m, kw = R.case_mask(n, h, w, mode)
    kw = {k: c.inp(torch.from_numpy(np.ascontiguousarray(v))) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    pg, xg = c.inp(torch.from_numpy(params)), c.inp(torch.from_numpy(x))
    out = c.out("out", n, chn, h, w)
    hip.nca_step(xg, pg, chn, hidden, out=out, **kw)
    c.check("step", out, torch.from_numpy(R.step(x64, params, chn, hidden, m)), 1e-6)      # tests/test_nca_gpu.py: 1e-6 on a step, 1e-5 on dx
    ws = c.ws("workspace", c.L.maua_nca_bwd_workspace_bytes(n, chn, hidden, h, w))
    dx, grad = c.out("dx", n, chn, h, w), c.out("grad", hip.nca_param_count(chn, hidden))
    hip.nca_step_bwd(xg, c.inp(torch.from_numpy(g)), pg, chn, hidden, ws, True, dx=dx, **kw)
    hip.nca_grad_finish((n, chn, h, w), chn, hidden, c.inp(c.used(ws)), out=grad)
    dx64, dw1, db1, dw2 = R.step_bwd(x64, g.astype(np.float64), params, chn, hidden, m)
    c.check("dx", dx, torch.from_numpy(dx64), 1e-5)
    c.check("grad", grad, torch.from_numpy(np.concatenate([dw1.ravel(), db1, dw2.ravel()])), TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# the test
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    """The library behind a recording proxy (tests/test_engine_gpu.py: Recorder) for the module's duration: which entry points ran."""
    import hip
    real, called = hip.lib(), set()

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("maua_"):
                return fn

            def call(*a):
                called.add(name)
                return fn(*a)
            return call
    hip._lib = Recorder()
    yield hip, called
    hip._lib = real
    hip.conv_x3p_set_max_groups(0)


@pytest.fixture(autouse=True)
def _restore(recorded):
    hip, _ = recorded
    yield
    for k in _FORCED:
        plan.OVERRIDES.pop(k, None)
    plan.forward_to_library(hip.lib())
    hip.conv_arm_workspace(None)
    hip.conv_x3p_set_max_groups(0)


@pytest.mark.parametrize("entry", TABLE, ids=lambda e: e.id)
def test_contained(recorded, entry):
    hip, called = recorded
    called.clear()
    runs = []
    for fill in (0x00, 0xFF):
        c = Ctx(hip, fill)
        try:
            entry.fn(c, **entry.params)
            runs.append(c.finish())
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):   # a faulted device: nothing more is started on it
                pytest.exit(f"{entry.id}: {e}", returncode=3)
            raise
        hip.conv_arm_workspace(None)
    missing = set(entry.entries) - called
    assert not missing, f"the case declares entry points it did not call: {sorted(missing)}"
    (bits0, sizes), (bits1, _) = runs
    assert bits0.keys() == bits1.keys()
    differ = [k for k in bits0 if not torch.equal(bits0[k], bits1[k])]
    assert not differ, f"results depend on what lies beyond the inputs (guards of 0x00 against 0xFF): {differ}"
    print(f"{entry.id}: {', '.join(sizes)}: guards intact, bits equal under both fills")
