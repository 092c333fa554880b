// Guided Gram matrices (Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer"): for R spatial guides g_r[HW] of
// one style layer with activation F[C][HW]
//     G_r = scale_r X_r X_r^T,   X_r[c][p] = g_r[p] (F[c][p] - mu_r[c]),   mu_r = sum_p g_r[p]^2 F[:,p] / N_r  (covariance form, else 0)
// and the backward pass gf[c][p] (+)= sum_r coef_r g_r[p]^2 sum_k D_r[k][c] (F[k][p] - mu_r[k]).
//
// The tiles, slabs, fp64 fold, ledger record and backward pipeline are gram_terms.hpp's.  What this file plugs in:
// Forward: the tile pairs ti <= tj only, the region as the term, and the guide multiplied in while a stage is written to LDS.  On a
// diagonal tile both MFMA operands read the same staged values.  The finishing kernels apply scale_r (a device float) and mirror the upper
// triangle: exactly symmetric.  A (region, 64-pixel stage) whose guide values are all zero is neither loaded nor multiplied (the test is
// the same in every wave of the workgroup), so R hard segmentation masks cost about one pass of matrix work in total.  A region with
// scale_r == 0 (inactive) is not computed: its matrix is exact zeros.
// Backward: one run of stages per region, each staged as coef_r g_r^2 (F - mu_r) against D_r, F with 16-byte loads in its own order; a
// region whose guide is zero over the workgroup's 256 pixels (or whose coef_r is 0) is left out.
// For the fused engine: a finishing kernel that also forms D_r = grad_scale_r (G_r - T_r) and the layer's loss as one ledger record
// (gg_finish_mse_kernel), and a ReLU mask in the backward kernel's epilogue (gg_bwd_kernel's MASK flag).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include "gram_terms.hpp"

namespace maua {

constexpr int GG_RMAX = 8;     // most regions per call
constexpr int GG_MSPLIT = 64;  // most partial sums per (region, row) of the weighted row means
constexpr int GG_KMAX = 256;   // most slabs per (region, tile pair)

static __host__ __device__ inline int gg_msplit(int64_t HW) {
    const int64_t k = (HW + 16383) / 16384;
    return k < 1 ? 1 : k > GG_MSPLIT ? GG_MSPLIT : (int)k;
}

// N_r = sum_p g_r[p]^2 in fp64: one workgroup per region, thread t adds the values t, t + 256, ... in order, then the fixed-order
// workgroup sum.  Runs once per set of guides.
__global__ void __launch_bounds__(256) gg_mass_kernel(const float* __restrict__ guides, double* __restrict__ mass, int64_t HW) {
    __shared__ double scratch[16];
    const float* g = guides + (int64_t)blockIdx.x * HW;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < HW; i += 256) {
        const double v = (double)g[i];
        acc += v * v;
    }
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) mass[blockIdx.x] = acc;
}

// Weighted row means in two fixed-order stages (as row_mean_partial_kernel / row_mean_finish_kernel): grid (C, splits, R) partial sums
// of g^2 F in fp64, then one thread per (region, row) adds that row's partial sums in index order and divides by N_r.
__global__ void __launch_bounds__(256) gg_mean_partial_kernel(const float* __restrict__ f, const float* __restrict__ guides,
                                                              const float* __restrict__ scale, double* __restrict__ partial, int C, int64_t HW) {
    __shared__ double scratch[16];
    const int c = blockIdx.x, part = blockIdx.y, r = blockIdx.z, split = gridDim.y;
    if (scale[r] == 0.f) return;  // (whole workgroup)
    const float* row = f + (int64_t)c * HW;
    const float* g = guides + (int64_t)r * HW;
    const int64_t per = (HW + split - 1) / split, lo = part * per, hi = min(HW, lo + per);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const double w = (double)g[i];
        acc += w * w * (double)row[i];
    }
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[((int64_t)r * C + c) * GG_MSPLIT + part] = acc;
}
__global__ void gg_mean_finish_kernel(const double* __restrict__ partial, const float* __restrict__ scale, const double* __restrict__ mass,
                                      float* __restrict__ mean, int C, int64_t HW) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (c >= C) return;
    float m = 0.f;
    if (scale[r] != 0.f) {
        double acc = 0.0;
        const int split = gg_msplit(HW);
        for (int k = 0; k < split; ++k) acc += partial[((int64_t)r * C + c) * GG_MSPLIT + k];
        m = (float)(acc / mass[r]);
    }
    mean[(int64_t)r * C + c] = m;
}

// One workgroup = one region x one upper-triangular 64x64 tile pair (ti <= tj) x one slice of HW.
__global__ void __launch_bounds__(256)
gg_partial_kernel(const float* __restrict__ f, const float* __restrict__ guides, const float* __restrict__ scale, const float* __restrict__ mean,
                  float* __restrict__ partial, int C, int64_t HW, int npairs, int ksplit, int64_t chunk) {
    __shared__ __attribute__((aligned(16))) float At[GT_T * GT_RS];
    __shared__ __attribute__((aligned(16))) float Bt[GT_T * GT_RS];
    const int reg = blockIdx.z;
    if (scale[reg] == 0.f) return;  // inactive region: the finishing kernel writes zeros without reading its slabs
    const int tid = threadIdx.x, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const bool diag = ti == tj;
    const int ks = blockIdx.y;
    const int64_t p_begin = (int64_t)ks * chunk;
    const int64_t p_end = min(HW, p_begin + chunk);
    const float* g = guides + (int64_t)reg * HW;
    const float* mu = mean ? mean + (int64_t)reg * C : nullptr;

    constexpr int NL = GT_T * GT_K / 4 / 256;
    const int r0 = tid >> 4, c4 = (tid & 15) * 4;
    float ma[NL], mb[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int rowa = ti * GT_T + r0 + 16 * q, rowb = tj * GT_T + r0 + 16 * q;
        ma[q] = (mu && rowa < C) ? mu[rowa] : 0.f;
        mb[q] = (mu && rowb < C) ? mu[rowb] : 0.f;
    }
    f32x4 ra[NL], rb[NL];
    // The guide quad of the stage after the one being loaded is requested a stage ahead, so the test below does not wait for memory.
    f32x4 gnext = p_begin < p_end ? gt_load4_end(g, p_begin + c4, p_end) : f32x4{0.f, 0.f, 0.f, 0.f};
    // -> true when the stage has a non-zero guide value; every wave's lanes 0 - 15 hold the stage's 64 guide values, so all four waves
    // of the workgroup decide alike and the barriers below stay matched
    auto load_stage = [&](int64_t p0) -> bool {
        const f32x4 gq = gnext;
        if (p0 + GT_K < p_end) gnext = gt_load4_end(g, p0 + GT_K + c4, p_end);
        const bool nz = gq[0] != 0.f || gq[1] != 0.f || gq[2] != 0.f || gq[3] != 0.f;
        if (__builtin_amdgcn_ballot_w64(nz) == 0ull) return false;
        const int64_t pp = p0 + c4;
        if (p0 + GT_K <= p_end && tj * GT_T + GT_T <= C) {  // workgroup-uniform: a whole stage of whole tiles, no per-load bounds
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                ra[q] = *reinterpret_cast<const gt_f32x4u*>(f + (int64_t)(ti * GT_T + r0 + 16 * q) * HW + pp);
                if (!diag) rb[q] = *reinterpret_cast<const gt_f32x4u*>(f + (int64_t)(tj * GT_T + r0 + 16 * q) * HW + pp);
            }
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                ra[q] = (ra[q] - ma[q]) * gq;
                if (!diag) rb[q] = (rb[q] - mb[q]) * gq;
            }
            return true;
        }
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int rowa = ti * GT_T + r0 + 16 * q, rowb = tj * GT_T + r0 + 16 * q;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            if (rowa < C) va = (gt_load4_end(f + (int64_t)rowa * HW, pp, p_end) - ma[q]) * gq;  // (cells beyond the slice: g = 0)
            if (!diag && rowb < C) vb = (gt_load4_end(f + (int64_t)rowb * HW, pp, p_end) - mb[q]) * gq;
            ra[q] = va;
            rb[q] = vb;
        }
        return true;
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            *reinterpret_cast<f32x4*>(At + (r0 + 16 * q) * GT_RS + c4) = ra[q];
            if (!diag) *reinterpret_cast<f32x4*>(Bt + (r0 + 16 * q) * GT_RS + c4) = rb[q];
        }
    };

    f32x16 acc = gt_zero16();
    const bool skip = diag && wi == 1 && wj == 0;  // wave-uniform: the mirrored block of a diagonal tile

    if (p_begin < p_end) {
        bool act_next = load_stage(p_begin);
        for (int64_t p0 = p_begin; p0 < p_end; p0 += GT_K) {
            const bool act = act_next;  // workgroup-uniform
            if (act) {
                __syncthreads();  // previous stage fully consumed
                store_stage();
                __syncthreads();
            }
            if (p0 + GT_K < p_end) act_next = load_stage(p0 + GT_K);
            if (act && !skip) gt_mma_stage(At, diag ? At : Bt, acc);
        }
    }
    gt_store_slab(partial, reg, npairs, ksplit, acc);
}

// grid (tile pairs, 16, R): every thread owns one element of the 64x64 tile, folds its slab values, applies the region's scale and writes
// the element and its mirror; the lower triangle of a diagonal tile is read from the upper one.
__global__ void __launch_bounds__(256)
gg_finish_kernel(const float* __restrict__ partial, const float* __restrict__ scale, float* __restrict__ gram, int C, int npairs, int ksplit) {
    const int reg = blockIdx.z;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int er = e / GT_T, ec = e % GT_T;
    const int src[1] = {(ti == tj && er > ec) ? ec * GT_T + er : e};
    const float sc = scale[reg];
    float s = 0.f;
    if (sc != 0.f) {
        double sd[1];
        gt_fold<8>(gt_slabs(partial, reg, npairs, ksplit), src, ksplit, sd);
        s = (float)(sd[0] * (double)sc);
    }
    const int gi = ti * GT_T + er, gj = tj * GT_T + ec;
    if (gi < C && gj < C) {
        float* gm = gram + (int64_t)reg * C * C;
        gm[(int64_t)gi * C + gj] = s;
        if (ti != tj) gm[(int64_t)gj * C + gi] = s;
    }
}

// gg_finish_kernel and the MSE against the regions' targets in one launch: grid (tile pairs, 16 / FQ, R), every thread owns FQ elements of
// the 64x64 tile (e = 256 (FQ blockIdx.y + u) + tid), folded exactly as gg_finish_kernel folds them (the same bits).
// D_r = grad_scale_r (G_r - T_r) is formed once per element of the upper triangle and written with its mirror (exactly symmetric whatever
// the target holds below its diagonal); exact zeros for a region with scale_r == 0 or grad_scale_r == 0.  The workgroup's share of
// loss_scale_r sum (G_r - T_r)^2 - off-diagonal tiles count twice - is one partial sum of the layer's ledger record (scale 1): R x pairs
// x 16 / FQ partial sums, a fixed order, no atomics.  The host takes the smallest FQ of 1, 2, 4 whose partial sums fit the record
// (gt_finish_split): FQ = 1 is gg_finish_kernel's grid - the serial chain of a thread is its slabs, so fewer, longer threads are slower
// where a layer has few tile pairs and many slabs - and FQ = 4 holds eight regions of 512 channels (8 x 36 x 4 sums).
template <int FQ>
__global__ void __launch_bounds__(256)
gg_finish_mse_kernel(const float* __restrict__ partial, const float* __restrict__ scale, float* __restrict__ gram, int C, int npairs, int ksplit,
                     const float* __restrict__ target, const float* __restrict__ loss_scale, const float* __restrict__ grad_scale,
                     float* __restrict__ dmat, double* __restrict__ rec) {
    constexpr int GG_FQ = FQ;
    const int reg = blockIdx.z;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const float sc = scale[reg], ls = loss_scale[reg], gs = grad_scale[reg];
    int er[GG_FQ], ec[GG_FQ], src[GG_FQ];
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) {
        const int e = (blockIdx.y * GG_FQ + u) * 256 + threadIdx.x;
        er[u] = e / GT_T;
        ec[u] = e % GT_T;
        src[u] = (ti == tj && er[u] > ec[u]) ? ec[u] * GT_T + er[u] : e;
    }
    float s[GG_FQ];
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) s[u] = 0.f;
    if (sc != 0.f) {
        double sd[GG_FQ];
        gt_fold<8>(gt_slabs(partial, reg, npairs, ksplit), src, ksplit, sd);
#pragma unroll
        for (int u = 0; u < GG_FQ; ++u) s[u] = (float)(sd[u] * (double)sc);
    }
    const bool with_d = sc != 0.f && gs != 0.f;
    const int64_t mat = (int64_t)reg * C * C;
    double sq = 0.0;
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) {
        const int gi = ti * GT_T + er[u], gj = tj * GT_T + ec[u];
        if (gi < C && gj < C) {
            // the element of the upper triangle this one mirrors (itself unless it lies below the diagonal of a diagonal tile)
            const bool low = ti == tj && er[u] > ec[u];
            const int64_t up = low ? (int64_t)gj * C + gi : (int64_t)gi * C + gj;
            float d = 0.f;
            if (with_d || ls != 0.f) d = s[u] - target[mat + up];
            const float dv = with_d ? gs * d : 0.f;
            gram[mat + (int64_t)gi * C + gj] = s[u];
            dmat[mat + (int64_t)gi * C + gj] = dv;
            if (ti != tj) {
                gram[mat + (int64_t)gj * C + gi] = s[u];
                dmat[mat + (int64_t)gj * C + gi] = dv;
            }
            if (ls != 0.f) sq += (ti != tj ? 2.0 : 1.0) * ((double)d * (double)d);
        }
    }
    gt_ledger_put(sq, reg, npairs, rec, [&](double sum) { return sum * (double)ls; });
}

// Backward: the stage runs are the regions.
template <bool ACC, bool MASK>
__global__ void __launch_bounds__(256)
gg_bwd_kernel(const float* __restrict__ d, const float* __restrict__ f, const float* __restrict__ guides, const float* __restrict__ coef,
              const float* __restrict__ mean, const float* __restrict__ relu_mask, float* __restrict__ gf, int R, int C, int64_t HW) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[32][256] + Wl[32][64])
    float* smem = smem_f32;
    constexpr int BUF = GTB_KC * GTB_PX + GTB_KC * GTB_CO;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * GTB_PX;
    const int co0 = blockIdx.y * GTB_CO;
    const int64_t pq = p0 + 4 * (tid & 63);  // this thread's pixel quad in every stage (each wave's 64 lanes cover the 256 pixels)

    // regions that take part: coef != 0 and a non-zero guide value among the workgroup's pixels (the same answer in every wave)
    unsigned active = 0;
    for (int r = 0; r < R; ++r) {
        const f32x4 gq = gt_load4_end(guides + (int64_t)r * HW, pq, HW);
        const bool nz = gq[0] != 0.f || gq[1] != 0.f || gq[2] != 0.f || gq[3] != 0.f;
        if (__builtin_amdgcn_ballot_w64(nz) != 0ull && coef[r] != 0.f) active |= 1u << r;
    }

    f32x4 rx[8], rw[2];
    auto load_stage = [&](int r, int k0) {
        const f32x4 gq = gt_load4_end(guides + (int64_t)r * HW, pq, HW);
        const float cf = coef[r];
        const f32x4 wq = gq * gq * cf;
        const float* dr = d + (int64_t)r * C * C;
        const float* mu = mean ? mean + (int64_t)r * C : nullptr;
        if (p0 + GTB_PX <= HW && k0 + GTB_KC <= C) {  // workgroup-uniform: 32 whole rows of 256 pixels, no per-load bounds
#pragma unroll
            for (int i = 0; i < 8; ++i) rx[i] = *reinterpret_cast<const gt_f32x4u*>(f + (int64_t)(k0 + (tid >> 6) + 4 * i) * HW + pq);
#pragma unroll
            for (int i = 0; i < 8; ++i) rx[i] = (rx[i] - (mu ? mu[k0 + (tid >> 6) + 4 * i] : 0.f)) * wq;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = k0 + (tid >> 6) + 4 * i;  // quad index tid + 256 i: 32 rows x 64 quads
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = (gt_load4_end(f + (int64_t)row * HW, pq, HW) - (mu ? mu[row] : 0.f)) * wq;  // (pixels beyond the plane: w = 0)
                rx[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i;  // 32 rows x 16 quads
            const int row = k0 + (e >> 4), q = e & 15;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < C) v = gt_load4_end(dr + (int64_t)row * C, co0 + 4 * q, C);
            rw[i] = v;
        }
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* wl = xl + GTB_KC * GTB_PX;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(xl + (tid + 256 * i) * 4) = rx[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(wl + (tid + 256 * i) * 4) = rw[i];
    };
    gt_bwd_run<ACC, MASK>(smem, active, R, C, HW, p0, co0, relu_mask, gf, load_stage, store_stage);
}

static bool gg_shape_ok(int regions, int c, int64_t hw) { return gt_shape_ok(regions, GG_RMAX, c, hw); }

}  // namespace maua

using namespace maua;

extern "C" {

int maua_gram_guided_supported(int regions, int c, int64_t hw) { return gg_shape_ok(regions, c, hw) ? 1 : 0; }

size_t maua_gram_guided_workspace_bytes(int regions, int c, int64_t hw) {
    if (!gg_shape_ok(regions, c, hw)) return 0;
    const size_t slabs = gt_plan(c, hw, false, GG_KMAX).slab_bytes(regions);
    const size_t mean_partials = (size_t)regions * c * GG_MSPLIT * sizeof(double);  // covariance form: used before the slabs
    return slabs > mean_partials ? slabs : mean_partials;
}

int maua_gram_guided_mass(const float* guides, double* mass, int regions, int64_t hw, maua_stream_t stream) {
    MAUA_REQUIRE(guides && mass, MAUA_E_INVAL, "gram_guided_mass: null pointer");
    MAUA_REQUIRE(gg_shape_ok(regions, 1, hw), MAUA_E_UNSUPPORTED, "gram_guided_mass: %d regions (1 .. %d) of %lld pixels", regions, GG_RMAX,
                 (long long)hw);
    hipLaunchKernelGGL(gg_mass_kernel, dim3(regions), dim3(256), 0, (hipStream_t)stream, guides, mass, hw);
    return check_launch("gg_mass_kernel");
}

// maua_gram_guided_fwd; with `mse` the finishing launch is gg_finish_mse_kernel
struct GuidedMse {
    const float *target, *loss_scale, *grad_scale;
    float* dmat;
    double* rec;
};
static int gg_forward(const char* who, const float* f, const float* guides, const float* scale, const double* mass, float* gram, float* mean_out,
                      int regions, int c, int64_t hw, int center, void* workspace, size_t workspace_bytes, const GuidedMse* mse,
                      maua_stream_t stream) {
    MAUA_REQUIRE(f && guides && scale && gram && workspace, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(!center || (mass && mean_out), MAUA_E_INVAL, "%s: center needs mass and mean_out", who);
    MAUA_REQUIRE(gg_shape_ok(regions, c, hw), MAUA_E_UNSUPPORTED, "%s: %d regions (1 .. %d), %d channels, %lld pixels", who, regions, GG_RMAX, c,
                 (long long)hw);
    MAUA_REQUIRE(!mse || maua_guided_gram_mse_ledger_supported(regions, c), MAUA_E_UNSUPPORTED,
                 "%s: %d regions of %d channels need more than %d partial sums", who, regions, c, LEDGER_MAX);
    const size_t need = maua_gram_guided_workspace_bytes(regions, c, hw);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    const GtPlan p = gt_plan(c, hw, false, GG_KMAX);
    hipStream_t s = (hipStream_t)stream;
    if (center) {
        // the partial sums live at the start of the workspace, which the slabs overwrite afterwards (same stream)
        hipLaunchKernelGGL(gg_mean_partial_kernel, dim3(c, gg_msplit(hw), regions), dim3(256), 0, s, f, guides, scale, (double*)workspace, c, hw);
        int rc = check_launch("gg_mean_partial_kernel");
        if (rc) return rc;
        hipLaunchKernelGGL(gg_mean_finish_kernel, dim3((c + 255) / 256, regions), dim3(256), 0, s, (const double*)workspace, scale, mass, mean_out,
                           c, hw);
        rc = check_launch("gg_mean_finish_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(gg_partial_kernel, dim3(p.npairs, p.ksplit, regions), dim3(256), 0, s, f, guides, scale, center ? mean_out : nullptr,
                       (float*)workspace, c, hw, p.npairs, p.ksplit, p.chunk);
    int rc = check_launch("gg_partial_kernel");
    if (rc) return rc;
    if (mse) {
        gt_launch_finish_mse(gg_finish_mse_kernel<1>, gg_finish_mse_kernel<2>, gg_finish_mse_kernel<4>, regions, p, s, (const float*)workspace, scale,
                             gram, c, p.npairs, p.ksplit, mse->target, mse->loss_scale, mse->grad_scale, mse->dmat, mse->rec);
        return check_launch("gg_finish_mse_kernel");
    }
    hipLaunchKernelGGL(gg_finish_kernel, dim3(p.npairs, GT_T * GT_T / 256, regions), dim3(256), 0, s, (const float*)workspace, scale, gram, c,
                       p.npairs, p.ksplit);
    return check_launch("gg_finish_kernel");
}

int maua_gram_guided_fwd(const float* f, const float* guides, const float* scale, const double* mass, float* gram, float* mean_out,
                         int regions, int c, int64_t hw, int center, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    return gg_forward("gram_guided_fwd", f, guides, scale, mass, gram, mean_out, regions, c, hw, center, workspace, workspace_bytes, nullptr, stream);
}

int maua_guided_gram_mse_ledger_supported(int regions, int c) {
    return gg_shape_ok(regions, c, 1) && gt_finish_split(regions, gt_pairs(c, false)) != 0 ? 1 : 0;
}

int maua_guided_gram_fwd_mse_ledger(const float* f, const float* guides, const float* scale, const double* mass, float* gram, float* mean_out,
                                    int regions, int c, int64_t hw, int center, const float* target, const float* loss_scale,
                                    const float* grad_scale, float* dmat, double* ledger, int slot, void* workspace, size_t workspace_bytes,
                                    maua_stream_t stream) {
    MAUA_REQUIRE(target && loss_scale && grad_scale && dmat && ledger && slot >= 0 && slot < (1 << 28), MAUA_E_INVAL,
                 "guided_gram_fwd_mse_ledger: bad args");
    const GuidedMse m{target, loss_scale, grad_scale, dmat, ledger + (int64_t)slot * LEDGER_STRIDE};
    return gg_forward("guided_gram_fwd_mse_ledger", f, guides, scale, mass, gram, mean_out, regions, c, hw, center, workspace, workspace_bytes, &m,
                      stream);
}

static int gg_backward(const char* who, const float* d_sym, const float* f, const float* guides, const float* coef, const float* mean,
                       const float* relu_mask, float* gf, int regions, int c, int64_t hw, int accumulate, maua_stream_t stream) {
    MAUA_REQUIRE(d_sym && f && guides && coef && gf, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(gg_shape_ok(regions, c, hw), MAUA_E_UNSUPPORTED, "%s: %d regions (1 .. %d), %d channels, %lld pixels", who, regions, GG_RMAX, c,
                 (long long)hw);
    gt_launch_bwd(gg_bwd_kernel<false, false>, gg_bwd_kernel<true, false>, gg_bwd_kernel<false, true>, gg_bwd_kernel<true, true>, accumulate != 0,
                  relu_mask != nullptr, c, hw, (hipStream_t)stream, d_sym, f, guides, coef, mean, relu_mask, gf, regions, c, hw);
    return check_launch("gg_bwd_kernel");
}

int maua_gram_guided_bwd(const float* d_sym, const float* f, const float* guides, const float* coef, const float* mean, float* gf, int regions,
                         int c, int64_t hw, int accumulate, maua_stream_t stream) {
    return gg_backward("gram_guided_bwd", d_sym, f, guides, coef, mean, nullptr, gf, regions, c, hw, accumulate, stream);
}

int maua_guided_gram_bwd_masked(const float* d_sym, const float* f, const float* guides, const float* coef, const float* mean,
                                const float* relu_mask, float* gf, int regions, int c, int64_t hw, int accumulate, maua_stream_t stream) {
    return gg_backward("guided_gram_bwd_masked", d_sym, f, guides, coef, mean, relu_mask, gf, regions, c, hw, accumulate, stream);
}

}  // extern "C"
