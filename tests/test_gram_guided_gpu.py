"""The guided Gram kernels (csrc/gram_guided.hip) against fp64, region by region.

Bar: rel-L2 <= 2e-5 relative to the region's own norm - TOL of tests/test_kernels_gpu.py for contractions.  The fp64 references are torch
matrix products on the device (independent of the kernels under test).  Inactive regions (mass < 1, scale 0) must give exact zeros,
every matrix must be exactly symmetric, and two runs must agree bit for bit."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = [(3, 5), (64, 1000), (96, 900), (128, 77), (512, 64), (256, 8100), (192, 5000), (1024, 961)]
REGIONS = [1, 2, 3, 8]
KINDS = ["hard", "empty", "skip", "soft", "ones"]


def hard_labels(N, R):
    """Region labels whose boundaries fall at pixels 255, 256 and 257 and at the start of every ragged last tile or stage (64 pixels in
    the forward kernel, 256 in the backward one) and at the last pixel."""
    cuts = sorted({p for p in (255, 256, 257, (N // 64) * 64, (N // 256) * 256, N - 1) if 0 < p < N})
    label = torch.zeros(N, dtype=torch.long)
    for p in cuts:
        label[p:] += 1
    return label % R


def make_guides(kind, R, N, gen):
    if kind == "ones":
        return torch.ones(R, N)
    if kind == "soft":
        return torch.rand(R, N, generator=gen)
    if kind == "skip":  # soft guides, region 0 zero over whole 64- and 256-pixel tiles at the front
        g = torch.rand(R, N, generator=gen)
        g[0, :320 if N > 320 else N // 2] = 0
        return g
    label = hard_labels(N, R)
    if kind == "empty":  # the last region owns no pixel
        label = torch.where(label == R - 1, torch.zeros_like(label), label) if R > 1 else label + 1
    return torch.stack([(label == r).float() for r in range(R)])


def reference(f, g, cov):
    """fp64 on the device: (grams (R,C,C), means (R,C), mass (R,), scale (R,))"""
    f64, g64 = f.double(), g.double()
    C = f.shape[0]
    mass = (g64 * g64).sum(1)
    grams, means, scale = [], [], []
    for r in range(g.shape[0]):
        act = bool(mass[r] >= 1.0)
        mu = (f64 * (g64[r] * g64[r])[None]).sum(1) / mass[r] if (cov and act) else torch.zeros(C, dtype=torch.float64, device=f.device)
        x = (f64 - mu[:, None]) * g64[r][None]
        sc = 1.0 / (C * float(mass[r])) if act else 0.0
        grams.append(x @ x.t() * sc)
        means.append(mu)
        scale.append(sc)
    return torch.stack(grams), torch.stack(means), mass, torch.tensor(scale, dtype=torch.float64, device=f.device)


def features(C, N, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(C, N, generator=gen) + 0.3), gen


@pytest.mark.parametrize("cov", [False, True], ids=["gram", "covariance"])
@pytest.mark.parametrize("R", REGIONS)
@pytest.mark.parametrize("C,N", SHAPES)
def test_guided_gram_forward_and_backward(C, N, R, cov):
    import hip
    f_cpu, gen = features(C, N, 1000 * R + C + N)
    f = f_cpu.cuda()
    for kind in KINDS:
        g = make_guides(kind, R, N, gen).cuda().contiguous()
        ref, ref_mean, ref_mass, ref_scale = reference(f, g, cov)
        mass = hip.gram_guided_mass(g)
        assert rel_l2(mass.cpu(), ref_mass.cpu()) <= 1e-12, kind
        scale = ref_scale.float()
        active = [bool(s != 0) for s in ref_scale]
        if kind == "empty":
            assert not active[-1]
        G, mean = hip.gram_guided_fwd(f, g, scale, cov, mass)
        G2, _ = hip.gram_guided_fwd(f, g, scale, cov, mass)
        torch.cuda.synchronize()
        assert torch.equal(G, G2), f"{kind}: two forward runs differ"
        for r in range(R):
            assert torch.equal(G[r], G[r].t()), f"{kind}: region {r} is not exactly symmetric"
            if not active[r]:
                assert not bool(G[r].any()), f"{kind}: inactive region {r} is not exact zeros"
                assert mean is None or not bool(mean[r].any())
                continue
            e = rel_l2(G[r].cpu(), ref[r].cpu())
            assert e <= TOL, f"{kind}: region {r} of {R}: rel-L2 {e:.3e}"
            if cov:
                assert rel_l2(mean[r].cpu(), ref_mean[r].cpu()) <= 1e-6, (kind, r)
        if kind == "ones" and R == 1:  # the unguided kernels on the same tensor
            plain, _ = hip.gram_fwd(f.reshape(1, C, 1, N), 1.0 / (C * N), cov)
            assert rel_l2(G[0].cpu(), plain.cpu()) <= TOL and rel_l2(plain.cpu(), ref[0].cpu()) <= TOL

        # backward: gf (+)= sum_r coef_r g_r^2 D_r (F - mu_r)
        d = torch.randn(R, C, C, generator=gen)
        d = (d + d.transpose(1, 2)).cuda().contiguous()
        want = torch.zeros(C, N, dtype=torch.float64, device="cuda")
        for r in range(R):
            if active[r]:
                want += float(ref_scale[r]) * (d[r].double() @ (f.double() - ref_mean[r][:, None])) * (g[r].double() ** 2)[None]
        # (the accumulate target has the size of what is added: acc - base below is then exact to fp32 rounding of the sum)
        base = torch.randn(C, N, generator=gen).cuda() * float(want.abs().max())
        gf = torch.full((C, N), float("nan"), device="cuda")
        hip.gram_guided_bwd(d, f, g, scale, mean, gf, False)
        gf2 = torch.full((C, N), float("nan"), device="cuda")
        hip.gram_guided_bwd(d, f, g, scale, mean, gf2, False)
        acc = base.clone()
        hip.gram_guided_bwd(d, f, g, scale, mean, acc, True)
        torch.cuda.synchronize()
        assert torch.equal(gf, gf2), f"{kind}: two backward runs differ"
        if not any(active):
            assert not bool(gf.any()) and torch.equal(acc, base), kind
            continue
        e = rel_l2(gf.cpu(), want.cpu())
        assert e <= TOL, f"{kind}: backward rel-L2 {e:.3e}"
        e = rel_l2((acc.double() - base.double()).cpu(), want.cpu())
        assert e <= TOL, f"{kind}: accumulating backward rel-L2 {e:.3e}"
        if kind in ("hard", "empty"):  # pixels of no active region get exactly nothing
            dead = (g[[r for r in range(R) if active[r]]] == 0).all(0)
            assert not bool(gf[:, dead].any())
            assert torch.equal(acc[:, dead], base[:, dead])


def test_refused_arguments_return_errors_and_launch_nothing():
    import hip
    L = hip.lib()
    C, N, R = 8, 100, 2
    f = torch.rand(C, N).cuda()
    g = torch.rand(R, N).cuda()
    scale = torch.full((R,), 0.01).cuda()
    mass = torch.full((R,), 30.0, dtype=torch.float64).cuda()
    gram = torch.full((9, C, C), 7.0).cuda()
    mean = torch.full((9, C), 7.0).cuda()
    gf = torch.full((C, N), 7.0).cuda()
    d = torch.zeros(9, C, C).cuda()
    need = L.maua_gram_guided_workspace_bytes(R, C, N)
    assert need > 0 and L.maua_gram_guided_supported(R, C, N) == 1
    ws = torch.zeros(need, dtype=torch.uint8).cuda()
    P = lambda t: t.data_ptr()  # noqa: E731
    S = hip._stream()
    for regions in (0, 9, -1):
        assert L.maua_gram_guided_supported(regions, C, N) == 0 and L.maua_gram_guided_workspace_bytes(regions, C, N) == 0
        assert L.maua_gram_guided_mass(P(g), P(mass), regions, N, S) < 0
        assert L.maua_gram_guided_fwd(P(f), P(g), P(scale), P(mass), P(gram), P(mean), regions, C, N, 1, P(ws), need, S) < 0
        assert L.maua_gram_guided_bwd(P(d), P(f), P(g), P(scale), P(mean), P(gf), regions, C, N, 0, S) < 0
    assert L.maua_gram_guided_supported(R, 0, N) == 0 and L.maua_gram_guided_supported(R, C, 0) == 0 and L.maua_gram_guided_supported(R, C, 1 << 30) == 0
    assert L.maua_gram_guided_mass(None, P(mass), R, N, S) < 0 and L.maua_gram_guided_mass(P(g), None, R, N, S) < 0
    for k in range(5):  # one null pointer at a time
        a = [P(f), P(g), P(scale), P(mass), P(gram)]
        if k == 3:
            continue  # (mass is nullable without centring; refused with it, below)
        a[k] = None
        assert L.maua_gram_guided_fwd(*a, P(mean), R, C, N, 0, P(ws), need, S) < 0, k
    assert L.maua_gram_guided_fwd(P(f), P(g), P(scale), None, P(gram), P(mean), R, C, N, 1, P(ws), need, S) < 0
    assert L.maua_gram_guided_fwd(P(f), P(g), P(scale), P(mass), P(gram), None, R, C, N, 1, P(ws), need, S) < 0
    assert L.maua_gram_guided_fwd(P(f), P(g), P(scale), P(mass), P(gram), P(mean), R, C, N, 1, None, need, S) < 0
    assert L.maua_gram_guided_fwd(P(f), P(g), P(scale), P(mass), P(gram), P(mean), R, C, N, 1, P(ws), need - 1, S) == -3
    assert b"workspace" in L.maua_last_error()
    for k in range(6):
        a = [P(d), P(f), P(g), P(scale), P(mean), P(gf)]
        if k == 4:
            continue  # (mean is nullable: no centring)
        a[k] = None
        assert L.maua_gram_guided_bwd(*a, R, C, N, 0, S) < 0, k
    torch.cuda.synchronize()
    assert bool((gram == 7).all()) and bool((mean == 7).all()) and bool((gf == 7).all()) and not bool(ws.any())
    assert float(mass[0]) == 30.0
