"""Record what the HOST half of the 3x3 convolution families decides - bank and workspace sizes, split-K factors, the routing
queries, and which calls the launch entry points refuse with which message - into tests/golden/conv_host_decisions.json.

    python tools/record_conv_host_decisions.py maua-style_amd/libmaua_hip.so

No GPU is needed or used: the queries are pure host arithmetic and every recorded launch call is one the argument checks turn
away before any HIP call (its return code is negative).  tests/test_conv_host_decisions_cpu.py recomputes the table with the
current build and demands equality, so the table is recorded BEFORE a change to that host code, from the commit it must match.

Layout of the file: {"vectors": [...], "index": {"<state>|<hint>|<query>": i}, "rejections": {...}}.  A vector is the query's
results over `shapes()` (or `channel_pairs()` for bank sizes) in order, as `encode()` packs it; identical vectors are stored once
(most queries do not read most tuning constants)."""
import hashlib
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_host_decisions.json")

CHANNELS = [3, 16, 22, 32, 48, 64, 96, 128, 256, 512]
PLANES = [1, 7, 16, 33, 64, 90, 128, 181, 256, 1024]
HINTS = [1, 4, 16]
# (tuning constant, values away from its default: the default itself is whatever the loaded library holds)
TUNINGS = [("x3w_ks", [2, 3, 5, 64]), ("x3q_ks", [2, 3, 5, 64]), ("x3p_ks", [2, 3, 5, 64]), ("x3q_min_fill", [0.5]), ("x3q_min_chunks", [8]),
           ("x3p_min_fill", [0.95]), ("x3p_min_items", [64]), ("x3p_groups", [64])]


def states():
    """(label, constant or None, value) - the defaults, then one constant at a time away from its default."""
    return [("default", None, None)] + [(f"{name}={v:g}", name, v) for name, values in TUNINGS for v in values]


def shapes():
    """(n, cin, h, w, cout, pad): the ordinary grid, shapes the routing queries prefer, then the degenerate ones."""
    out = []
    for n, cin, cout, p, pad in itertools.product([1, 4], CHANNELS, CHANNELS, PLANES, [0, 1, 2]):
        out += [(n, cin, p, p, cout, pad), (n, cin, p, p + 3, cout, pad)]
    out += [(1, 512, 128, 128, 512, 1), (1, 512, 90, 90, 512, 1), (1, 256, 256, 256, 256, 1), (1, 64, 512, 512, 64, 1), (1, 128, 512, 512, 128, 1),
            (1, 512, 64, 64, 512, 1), (1, 512, 32, 32, 512, 1), (16, 512, 32, 32, 512, 1), (1, 100, 64, 64, 100, 1), (1, 1024, 45, 45, 1024, 1)]
    big = 1 << 24
    for v in (0, -1, -7):  # zero and negative extents, one argument at a time
        for i in range(5):
            s = [1, 64, 32, 32, 64, 1]
            s[i] = v
            out.append(tuple(s))
    out += [(1, 64, 32, 32, 64, -1), (1, 64, 32, 32, 64, 3), (1, 64, 32, 32, 64, 64), (1, 64, 32, 32, 64, 65),
            (1, 64, 1, 1, 64, 0), (1, 64, 2, 2, 64, 0), (1, 64, 2, 9, 64, 0), (1, 64, 9, 2, 64, 0), (1, 64, 3, 3, 64, 0), (1, 64, 1, 1, 64, 1),
            (1 << 16, 64, 8, 8, 64, 1), ((1 << 16) + 1, 64, 8, 8, 64, 1), (1, 1 << 20, 8, 8, 64, 1), (1, (1 << 20) + 32, 8, 8, 64, 1),
            (1, 64, 8, 8, 1 << 20, 1), (1, 64, 8, 8, (1 << 20) + 64, 1), (1, 64, big, 8, 64, 1), (1, 64, big + 1, 8, 64, 1),
            (1, 64, 8, big, 64, 1), (1, 64, 8, big + 1, 64, 1), (1, 64, 32768, 32767, 64, 1), (1, 64, 32768, 32768, 64, 1),
            (1, 64, 4096, 4096, 64, 1), (1, 64, 4096, 4097, 64, 1), (1, 64, 5792, 5792, 64, 1), (1, 64, 5793, 5793, 64, 1),
            (1, 512, 1024, 1024, 512, 1), (1, 512, 1024, 1025, 512, 1),
            (2147483647, 2147483647, 2147483647, 2147483647, 2147483647, 2147483647), (1, 64, 2147483647, 1, 64, 2), (1, 64, 1, 2147483647, 64, 2)]
    return out


def channel_pairs():
    edge = [0, -1, 1, (1 << 20), (1 << 20) + 1, 2147483647]
    return list(itertools.product(CHANNELS + [100], CHANNELS + [100])) + [(a, 64) for a in edge] + [(64, a) for a in edge]


# query -> (exported function, its arguments from a shape (n, cin, h, w, cout, pad)); a bank size (None) runs over channel_pairs()
QUERIES = {f"maua_conv_{fam}_bank_bytes": None for fam in ("x6", "x3", "x3w", "x3q", "kxk_x3")}
QUERIES.update({name: (name, lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, pad)) for name in (
    "maua_conv_x6_workspace_bytes", "maua_conv_x3_workspace_bytes", "maua_conv_x3w_workspace_bytes", "maua_conv_x3w_split",
    "maua_conv_x3q_workspace_bytes", "maua_conv_x3q_split", "maua_conv_x3q_preferred", "maua_conv_x3p_workspace_bytes", "maua_conv_x3p_split",
    "maua_conv_x3p_preferred")})
QUERIES.update({
    "maua_conv_x3w_supported": ("maua_conv_x3w_supported", lambda n, cin, h, w, cout, pad: (cin, h, w, pad)),
    "maua_conv_x3q_supported": ("maua_conv_x3q_supported", lambda n, cin, h, w, cout, pad: (cin, h, w, pad)),
    "maua_conv_x3p_supported": ("maua_conv_x3p_supported", lambda n, cin, h, w, cout, pad: (cin, h, w, cout, pad)),
    "maua_conv_kxk_x3_workspace_bytes/5": ("maua_conv_kxk_x3_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 5, pad)),
    "maua_conv_kxk_x3_workspace_bytes/3": ("maua_conv_kxk_x3_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 3, pad)),
    "maua_conv_workspace_bytes/1": ("maua_conv_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 1, 1, 1, pad)),
    "maua_conv_workspace_bytes/3": ("maua_conv_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 3, 3, 1, pad)),
    "maua_conv_workspace_bytes/5": ("maua_conv_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 5, 5, 1, pad)),
    "maua_conv_workspace_bytes/3s2": ("maua_conv_workspace_bytes", lambda n, cin, h, w, cout, pad: (n, cin, h, w, cout, 3, 3, 2, pad)),
})


P = 0x10000  # fake non-null device pointer: host code only passes it on
OK = dict(n=1, cin=64, h=32, w=32, cout=64, pad=1)


def rejections(L):
    """[(label, thunk)]: calls every launch entry point must turn away before any HIP call."""
    out = []

    def add(entry, order, base, cases):
        f = getattr(L, entry)
        for label, change in cases:
            args = dict(base, **change)
            out.append((f"{entry}: {label}", (lambda f, a: lambda: f(*a))(f, [args[k] for k in order])))

    dims = [("n = 0", dict(n=0)), ("n < 0", dict(n=-2)), ("cin = 0", dict(cin=0)), ("cout = 0", dict(cout=0)), ("h = 0", dict(h=0)), ("w < 0", dict(w=-5)),
            ("pad < 0", dict(pad=-1)), ("pad = 3", dict(pad=3)), ("pad = 65", dict(pad=65)), ("n too large", dict(n=(1 << 16) + 1)),
            ("cin too large", dict(cin=(1 << 20) + 64)), ("cout too large", dict(cout=(1 << 20) + 64)), ("h too large", dict(h=(1 << 24) + 1)),
            ("plane of 2^30 pixels", dict(h=32768, w=32768)), ("extents at INT_MAX", dict(n=2147483647, cin=2147483647, h=2147483647, w=2147483647, cout=2147483647, pad=2147483647)),
            ("1 x 1 input, pad 0", dict(h=1, w=1, pad=0)), ("2 x 9 input, pad 0", dict(h=2, w=9, pad=0)), ("9 x 2 input, pad 0", dict(h=9, w=2, pad=0))]
    scale = [("w_scale = 0", dict(w_scale=0.0)), ("w_scale < 0", dict(w_scale=-1.0))]

    def nulls(*names):
        return [(f"null {k}", {k: None}) for k in names]

    plain = ["x", "bank", "w_scale", "bias", "omask", "y", "n", "cin", "h", "w", "cout", "pad", "relu", "acc", "ws", "wsb", "stream"]
    base = dict(OK, x=P, bank=P, w_scale=1.0, bias=P, omask=None, y=P, relu=1, acc=0, ws=None, wsb=0, stream=None)
    add("maua_conv3x3_x6", [k for k in plain if k != "w_scale"], base, nulls("x", "bank", "y") + dims)
    add("maua_conv3x3_x3", plain, base, nulls("x", "bank", "y") + scale + dims)
    add("maua_conv3x3_x3w", plain, base, nulls("x", "bank", "y") + scale + dims + [("cin = 24", dict(cin=24)), ("cin = 3", dict(cin=3)), ("plane above 2^25", dict(h=8192, w=4097))])
    add("maua_conv3x3_x3q", plain, base, nulls("x", "bank", "y") + scale + dims + [("cin = 48", dict(cin=48)), ("cin = 16", dict(cin=16)), ("plane above 2^24", dict(h=4096, w=4097))])
    pool = ["x", "bank", "w_scale", "bias", "pooled", "codes", "n", "cin", "h", "w", "cout", "pad", "ws", "wsb", "stream"]
    pbase = dict(base, pooled=P, codes=P)
    pool_cases = nulls("x", "bank", "pooled", "codes") + scale + dims + [("3 x 3 input, pad 0: 1 x 1 output", dict(h=3, w=3, pad=0)), ("cout = 60", dict(cout=60)),
                                                                          ("cout = 3", dict(cout=3))]
    add("maua_conv3x3_x3w_relu_pool", pool, pbase, pool_cases + [("cin = 24", dict(cin=24))])
    add("maua_conv3x3_x3q_relu_pool", pool, pbase, pool_cases + [("cin = 48", dict(cin=48)), ("plane above 2^24", dict(h=4096, w=4097))])
    gram = ["x", "bank", "w_scale", "fmap", "dbank", "dinv", "y", "n", "cin", "h", "w", "cout", "pad", "acc", "ws", "wsb", "stream"]
    add("maua_conv3x3_x3w_gram", gram, dict(base, fmap=P, dbank=P, dinv=P),
        nulls("x", "bank", "y", "dbank", "dinv", "fmap") + scale + dims + [("cin = 24", dict(cin=24)), ("cout = 24", dict(cout=24)), ("pad = 0: smaller output plane", dict(pad=0)),
                                                                           ("pad = 2: larger output plane", dict(pad=2))])
    unw = ["x", "codes", "honour", "bank", "w_scale", "omask", "dbank", "dinv", "y", "n", "cin", "h", "w", "cout", "pad", "ws", "wsb", "stream"]
    ubase = dict(base, codes=P, honour=1, dbank=None, dinv=None)
    un_cases = nulls("x", "codes", "bank", "y") + scale + dims + [("1 x 4 input, pad 1", dict(h=1, w=4)), ("4 x 1 input, pad 1", dict(h=4, w=1))]
    add("maua_conv3x3_x3w_unpool", unw, ubase, un_cases + [("cin = 24", dict(cin=24)), ("Gram bank without its inverse scale", dict(dbank=P, omask=P)),
                                                           ("Gram bank without the feature map", dict(dbank=P, dinv=P)),
                                                           ("Gram bank, cout = 24", dict(dbank=P, dinv=P, omask=P, cout=24)), ("Gram bank, pad 0", dict(dbank=P, dinv=P, omask=P, pad=0))])
    add("maua_conv3x3_x3q_unpool", [k for k in unw if k not in ("dbank", "dinv")], ubase, un_cases + [("cin = 48", dict(cin=48))])
    x3p = ["x", "in_codes", "honour", "bank", "w_scale", "bias", "omask", "dbank", "dinv", "y", "pool_codes", "n", "cin", "h", "w", "cout", "pad", "relu", "ws", "wsb", "stream"]
    add("maua_conv3x3_x3p", x3p, dict(base, in_codes=None, honour=1, dbank=None, dinv=None, pool_codes=None),
        nulls("x", "bank", "y") + scale + dims + [("cin = 48", dict(cin=48)), ("cout = 96", dict(cout=96)), ("cout = 576", dict(cout=576)), ("plane above 2^24", dict(h=4096, w=4097)),
                                                  ("output image of 2 GiB", dict(cout=512, h=1024, w=1024)), ("pool: 3 x 3 input, pad 0", dict(pool_codes=P, h=3, w=3, pad=0)),
                                                  ("pool with a mask", dict(pool_codes=P, omask=P)), ("pool with a Gram bank", dict(pool_codes=P, dbank=P, dinv=P)),
                                                  ("pool with unpool", dict(pool_codes=P, in_codes=P)), ("pool without ReLU", dict(pool_codes=P, relu=0)),
                                                  ("Gram without the inverse scale", dict(dbank=P, omask=P)), ("Gram without the feature map", dict(dbank=P, dinv=P)),
                                                  ("Gram, pad 0", dict(dbank=P, dinv=P, omask=P, pad=0)), ("unpool: 1 x 4 input", dict(in_codes=P, h=1, w=4)),
                                                  ("unpool: 4 x 1 input", dict(in_codes=P, h=4, w=1))])
    kxk = ["x", "bank", "w_scale", "bias", "omask", "y", "n", "cin", "h", "w", "cout", "ks", "pad", "relu", "acc", "ws", "wsb", "stream"]
    add("maua_conv_kxk_x3", kxk, dict(base, ks=5, pad=2), nulls("x", "bank", "y") + scale + [d for d in dims if d[0] != "pad = 3"] +
        [("ks = 3", dict(ks=3)), ("ks = 7", dict(ks=7)), ("ks = 0", dict(ks=0)), ("pad = 5", dict(pad=5)), ("4 x 4 input, pad 0", dict(h=4, w=4, pad=0)),
         ("plane of 2^29 pixels", dict(h=32768, w=16384))])
    pack = ["w", "bf", "bb", "cout", "cin", "w_scale", "stream"]
    pk = dict(w=P, bf=P, bb=P, cout=64, cin=64, w_scale=1.0, ks=5, stream=None)
    pack_cases = [("null weights", dict(w=None)), ("no bank", dict(bf=None, bb=None)), ("cout = 0", dict(cout=0)), ("cin < 0", dict(cin=-1)),
                  ("cout too large", dict(cout=(1 << 20) + 1)), ("cin too large", dict(cin=(1 << 20) + 1))]
    add("maua_conv_pack_filters_x6", [k for k in pack if k != "w_scale"], pk, pack_cases)
    for fam in ("x3", "x3w", "x3q"):
        add(f"maua_conv_pack_filters_{fam}", pack, pk, pack_cases + scale)
    add("maua_conv_pack_filters_kxk_x3", ["w", "bf", "bb", "cout", "cin", "ks", "w_scale", "stream"], pk, pack_cases + scale + [("ks = 0", dict(ks=0))])
    fwd = ["x", "mask", "wf", "bias", "y", "n", "cin", "h", "w", "cout", "kh", "kw", "stride", "pad", "relu", "acc", "ws", "wsb", "stream"]
    gen = [d for d in dims if d[0] not in ("pad = 3", "plane of 2^30 pixels")] + [("kh = 0", dict(kh=0)), ("kw = 65", dict(kw=65)), ("stride = 0", dict(stride=0)),
                                                                                  ("stride = 65", dict(stride=65))]
    add("maua_conv2d_fwd", fwd, dict(base, mask=None, wf=P, kh=3, kw=3, stride=1), nulls("x", "wf", "y") + gen)
    bwd = ["gy", "mask", "wb", "w_oihw", "omask", "gx", "n", "cin", "h", "w", "cout", "kh", "kw", "stride", "pad", "acc", "ws", "wsb", "stream"]
    add("maua_conv2d_bwd_data", bwd, dict(base, gy=P, mask=None, wb=P, w_oihw=None, gx=P, kh=3, kw=3, stride=1),
        nulls("gy", "gx", "wb") + gen + [("pad = 3 > k - 1", dict(pad=3)), ("direct path without OIHW weights", dict(stride=2))])
    return out


def encode(values):
    """Run-length encoded [value, count, ...] where that is short (splits, yes / no answers); else - byte counts that differ from
    shape to shape - {"sha1": the first 10 hex digits of the SHA-1 of each block of 256 values, "distinct": 2 if two values differ}."""
    out = []
    for v in values:
        if out and out[-2] == v:
            out[-1] += 1
        else:
            out += [v, 1]
    if len(out) <= 800:
        return out
    blocks = [hashlib.sha1(repr(values[i:i + 256]).encode()).hexdigest()[:10] for i in range(0, len(values), 256)]
    return {"sha1": blocks, "distinct": min(2, len(set(values)))}


def compute(L):
    """The whole table with library `L` (hip.lib()): every query over every shape and every refusal, under every state and hint.
    Only the constant a state moves is set, and it goes back to the value it had; so does the batch hint."""
    sh, pairs = shapes(), channel_pairs()
    calls = {q: None if v is None else (getattr(L, v[0]), [v[1](*s) for s in sh]) for q, v in QUERIES.items()}
    hint_before = L.maua_get_split_batch_hint()
    vectors, where, index, rej = [], {}, {}, {}
    for label, moved, value in states():
        if moved:
            held = L.maua_get_tuning(moved.encode(), float("nan"))
            assert held == held, f"{moved} was never handed to the library: its default is not known here"
            L.maua_set_tuning(moved.encode(), float(value))
        try:
            for hint in HINTS:
                L.maua_set_split_batch_hint(hint)
                for qname, call in calls.items():
                    if call is None:
                        f = getattr(L, qname)
                        vals = [f(co, ci, 5) for co, ci in pairs] if "kxk" in qname else [f(co, ci) for co, ci in pairs]
                    elif moved == "x3p_ks" and qname in ("maua_conv_x3p_split", "maua_conv_x3p_workspace_bytes"):
                        # (with its split forced, the persistent family's cost model divides by zero below one 32-channel chunk: not called)
                        vals = [call[0](*t) if t[1] >= 32 else -1 for t in call[1]]
                    else:
                        f = call[0]
                        vals = [f(*t) for t in call[1]]
                    key = json.dumps(encode(vals), separators=(",", ":"))
                    if key not in where:
                        where[key] = len(vectors)
                        vectors.append(json.loads(key))
                    index[f"{label}|{hint}|{qname}"] = where[key]
                got = {}
                for rlabel, thunk in rejections(L):
                    rc = thunk()
                    got[rlabel] = [rc, L.maua_last_error().decode(errors="replace")]
                rej[f"{label}|{hint}"] = got
        finally:
            if moved:
                L.maua_set_tuning(moved.encode(), held)
            L.maua_set_split_batch_hint(hint_before)
    # the refusals do not depend on the planner's state: stored once, with the states that differ (none expected) next to it
    first = rej["default|1"]
    return {"shapes": len(sh), "channel_pairs": len(pairs), "vectors": vectors, "index": index, "rejections": first,
            "rejections_elsewhere": {k: v for k, v in rej.items() if v != first}}


def main():
    os.environ["MAUA_HIP_LIB"] = os.path.abspath(sys.argv[1])
    sys.path[:0] = [os.path.join(REPO, "maua-style_amd")]
    import hip
    table = compute(hip.lib())
    bad = {k: v for k, v in table["rejections"].items() if v[0] >= 0}
    assert not bad, f"calls that were meant to be refused got past the argument checks: {bad}"
    text = json.dumps(table, separators=(",", ":"))
    assert len(text) < 256 * 1024, len(text)
    with open(GOLDEN, "w") as f:
        f.write(text + "\n")
    print(f"{GOLDEN}: {len(text)} bytes, {len(table['vectors'])} distinct vectors, {len(table['index'])} entries, {len(table['rejections'])} refusals")


if __name__ == "__main__":
    main()
