"""Shape fuzzer for the host half of the neural cellular automaton entry points (maua_nca_*), run against the host-sanitised build
(ASan + UBSan on the host code, device code plain) without a GPU:

    python maua-style_amd/build_native.py --sanitize
    LD_PRELOAD=<clang_rt.asan> python tools/fuzz_nca_host.py LIB [N] [SEED]

Pointers are fake non-null addresses that host code only passes on.  What must hold: no sanitizer report, size functions consistent
with the support predicate, invalid arguments answered with a negative code before any launch."""
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "maua-style_amd")]


def main():
    lib_path = sys.argv[1]
    n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    rng = random.Random(int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    os.environ["MAUA_HIP_LIB"] = lib_path
    import hip
    L = hip.lib()
    P = 0x10000
    edge = [-7, -1, 0, 1, 2, 3, 5, 8, 12, 16, 96, 127, 128, 129, 4096, 16384, 16385, 65536, 65537, 1 << 20, (1 << 31) - 1]
    pairs = [(12, 96), (16, 128), (12, 128), (0, 0), (-12, 96), (1 << 30, 96)]
    for _ in range(n_cases):
        n, h, w = (rng.choice(edge) if rng.random() < 0.7 else rng.randint(-3, 5000) for _ in range(3))
        chn, hidden = rng.choice(pairs)
        ok = L.maua_nca_supported(n, chn, hidden, h, w)
        ws = L.maua_nca_bwd_workspace_bytes(n, chn, hidden, h, w)
        pc = L.maua_nca_param_count(chn, hidden)
        assert (ws > 0) == bool(ok), (n, chn, hidden, h, w, ws)
        assert pc >= 0 and (pc > 0) == ((chn, hidden) in ((12, 96), (16, 128)))
        if ok:
            assert n * h * w <= 1 << 28 and ws >= n * 4 * chn * h * w * 4
            continue  # a valid shape would launch; the GPU-less host has nothing to run it on
        step = rng.choice([0, 1, -1, 1 << 40])
        assert L.maua_nca_step(P, P + 64, P, n, chn, hidden, h, w, 0.5, None, None, rng.getrandbits(64), step, None) < 0
        assert L.maua_nca_step_bwd(P, P + 64, P + 128, P, n, chn, hidden, h, w, 0.5, None, None, 7, step, 1, P,
                                   rng.choice([0, 1, 1 << 40]), None) < 0
        assert L.maua_nca_grad_finish(P, n, chn, hidden, h, w, P, rng.choice([0, 1 << 40]), 1, None) < 0
    print(f"{n_cases} cases: no sanitizer report")


if __name__ == "__main__":
    main()
