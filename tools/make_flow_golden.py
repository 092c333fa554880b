"""Write tests/golden/flow_consistency.npz: the reference's own check_consistency and flow_to_image (flow.py:77-220) on a set of
flow pairs, for tests/test_flow_cpu.py and tests/test_flow_gpu.py (read through tests/flow_restatement.py:fixture_cases).  The
flows are multiples of 2^-shift (shift <= 6) stored exactly as int16 differences along each row (`q1_i`, `q2_i`, `shift_i`),
which keeps the file small.

Runs where the reference checkout exists (argument 1, default ../reference next to this repository), never from a test.  Importing
the reference's flow.py is not possible (at import time it rewrites files of its network submodules), so the four functions are
taken from the UNMODIFIED file with `ast` and executed against numpy / scipy as installed, with one shim: `np.int`, removed from
numpy 1.24, is the builtin int it always was an alias of.

    python tools/make_flow_golden.py [/path/to/reference]
"""
import ast
import os
import sys
import types

import numpy as np
import scipy
import scipy.ndimage  # noqa: F401  (the reference calls scipy.ndimage.gaussian_filter through `import scipy`)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ("check_consistency", "flow_to_image", "compute_color", "make_color_wheel")


def reference_functions(ref_root):
    src = open(os.path.join(ref_root, "flow.py")).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert sorted(n.name for n in keep) == sorted(WANT), [n.name for n in keep]
    shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    shim.int = int
    # scipy as installed, with gaussian_filter observed on the way through: its input is the reference's classification (1 reliable,
    # -1 round trip inconsistent, 0 outside the frame / motion edge) before the blur
    seen = []

    def gaussian_filter(a, *args, **kwargs):
        seen.append(np.array(a))
        return scipy.ndimage.gaussian_filter(a, *args, **kwargs)
    sp = types.SimpleNamespace(ndimage=types.SimpleNamespace(gaussian_filter=gaussian_filter))
    ns = {"np": shim, "scipy": sp, "_seen": seen}
    exec(compile(ast.Module(body=keep, type_ignores=[]), os.path.join(ref_root, "flow.py"), "exec"), ns)
    return ns


def grid(h, w):
    y, x = np.mgrid[:h, :w].astype(np.float64)
    return x, y


def pair_translation(h, w, du, dv):
    f = np.zeros((h, w, 2), np.float32)
    f[..., 0], f[..., 1] = du, dv
    return f, -f


def pair_occluder(h, w, rng):
    """Static background, a square moving by (du, dv): forward flow on the square, backward flow on its moved position."""
    s = max(2, min(h, w) // 3)
    y0, x0 = (h - s) // 3, (w - s) // 3
    du, dv = float(rng.uniform(3, 6)), float(rng.uniform(-4, -1))
    f1 = (rng.normal(size=(h, w, 2)) * 0.004).astype(np.float32)
    f2 = (rng.normal(size=(h, w, 2)) * 0.004).astype(np.float32)
    f1[y0:y0 + s, x0:x0 + s] = (du, dv)
    ys, xs = int(round(y0 + dv)), int(round(x0 + du))
    f2[max(ys, 0):max(ys + s, 0), max(xs, 0):max(xs + s, 0)] = (-du, -dv)
    return f1, f2


def pair_rotation_zoom(h, w, angle, zoom):
    """x -> A (x - c) + c and its exact inverse."""
    x, y = grid(h, w)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    c, s = np.cos(angle) * zoom, np.sin(angle) * zoom
    A = np.array([[c, -s], [s, c]])
    Ai = np.linalg.inv(A)

    def field(M):
        px, py = x - cx, y - cy
        return np.stack([M[0, 0] * px + M[0, 1] * py - px, M[1, 0] * px + M[1, 1] * py - py], axis=2).astype(np.float32)
    return field(A), field(Ai)


def pair_leaving(h, w, rng):
    """Smooth flow that carries the right part of the frame out of it, plus noise (motion edges)."""
    x, y = grid(h, w)
    f1 = np.stack([0.6 * w * (x / max(w - 1, 1)) ** 2, 1.5 * np.sin(y / 7.0)], axis=2)
    f1 = (f1 + rng.normal(size=f1.shape) * 0.05).astype(np.float32)
    return f1, (-f1 + rng.normal(size=f1.shape).astype(np.float32) * 0.3).astype(np.float32)


def quantised(f):
    """(int16 field, shift) with f ~ field * 2^-shift: the flows of the fixture are exactly such values (in float32), so they are
    stored in two bytes each; shift <= 6, and max |f| * 2^shift stays below 2^15."""
    shift = 14 - int(np.ceil(np.log2(max(float(np.abs(f).max()), 1e-3) + 1e-9)))
    shift = max(0, min(shift, 6))  # (1/64 px steps: plenty for the decisions, and the arrays compress)
    return np.rint(f.astype(np.float64) * 2.0 ** shift).astype(np.int16), shift


def cases(rng):
    """Odd sides, 2 x N, N x 2 and sides under 41 (where the 41 x 41 erosion leaves nothing reliable: the last row and column always
    map to the frame's edge, which counts as outside), and frames large enough for both mask values to cover much of them."""
    out = []
    for h, w in ((75, 61), (33, 47), (2, 50), (50, 2), (17, 23)):
        out.append(("translation", pair_translation(h, w, 3.3, -1.7)))
        out.append(("occluder", pair_occluder(h, w, rng)))
        out.append(("rotation_zoom", pair_rotation_zoom(h, w, 0.05, 1.03)))
        out.append(("leaving", pair_leaving(h, w, rng)))
    out.append(("translation", pair_translation(112, 128, 3.3, -1.7)))
    out.append(("translation_subpixel", pair_translation(99, 121, 0.4, 0.25)))
    out.append(("occluder", pair_occluder(121, 112, rng)))
    out.append(("rotation_zoom", pair_rotation_zoom(112, 127, 0.004, 1.002)))
    out.append(("leaving", pair_leaving(96, 112, rng)))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(REPO), "reference")
    fns = reference_functions(ref)
    rng = np.random.default_rng(20261015)
    data, kinds = {}, []
    for i, (kind, (f1, f2)) in enumerate(cases(rng)):
        (q1, s1), (q2, s2) = quantised(f1), quantised(f2)
        f1 = (q1.astype(np.float64) * 2.0 ** -s1).astype(np.float32)  # exact: these are the flows the reference sees
        f2 = (q2.astype(np.float64) * 2.0 ** -s2).astype(np.float32)
        fns["_seen"].clear()
        r = fns["check_consistency"](f1.copy(), f2.copy())
        # stored as differences along rows (smooth fields compress to almost nothing); fixture_cases takes the cumulative sum
        data[f"q1_{i}"], data[f"q2_{i}"] = np.diff(q1, axis=1, prepend=0), np.diff(q2, axis=1, prepend=0)
        data[f"shift_{i}"] = np.array([s1, s2], np.int32)
        data[f"class_{i}"] = fns["_seen"][0].astype(np.int8)
        data[f"mask_{i}"] = ((1 - r) * 255).astype(np.uint8)  # what load.process_content_video saves (load.py:176-177)
        data[f"color_{i}"] = fns["flow_to_image"](f1.copy())
        kinds.append(kind)
        print(f"{i:2d} {kind:18s} {f1.shape[0]}x{f1.shape[1]}  reliable {float(r.mean()):.3f}  classes -1/0/1 "
              f"{[int((data[f'class_{i}'] == c).sum()) for c in (-1, 0, 1)]}")
    data["kinds"] = np.array(kinds)
    data["numpy_version"], data["scipy_version"] = np.array(np.__version__), np.array(scipy.__version__)
    path = os.path.join(REPO, "tests", "golden", "flow_consistency.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
