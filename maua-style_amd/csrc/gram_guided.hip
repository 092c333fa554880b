// Guided Gram matrices (Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style Transfer"): for R spatial guides g_r[HW] of
// one style layer with activation F[C][HW]
//     G_r = scale_r X_r X_r^T,   X_r[c][p] = g_r[p] (F[c][p] - mu_r[c]),   mu_r = sum_p g_r[p]^2 F[:,p] / N_r  (covariance form, else 0)
// and the backward pass gf[c][p] (+)= sum_r coef_r g_r[p]^2 sum_k D_r[k][c] (F[k][p] - mu_r[k]).
//
// Forward: gram.hip's fp32-MFMA split-K kernel with one more grid dimension (the region) and the guide multiplied in while a stage is
// written to LDS - both MFMA operands read the same staged values, the finishing kernel adds the slabs in index order (fp64), applies
// scale_r and mirrors the upper triangle: deterministic, exactly symmetric, no float atomics.  A (region, 64-pixel stage) whose guide
// values are all zero is neither loaded nor multiplied (the test is the same in every wave of the workgroup), so R hard segmentation
// masks cost about one pass of matrix work in total.  A region with scale_r == 0 (inactive) is not computed: its matrix is exact zeros.
// Backward: gram_bwd_kernel's layout (64 output channels x 256 pixels per workgroup, F staged with 16-byte loads in its own order); the
// regions are further stages of the same accumulation, each staged as coef_r g_r^2 (F - mu_r) against D_r, and a region whose guide is
// zero over the workgroup's 256 pixels (or whose coef_r is 0) is left out.
// For the fused engine: a finishing kernel that also forms D_r = grad_scale_r (G_r - T_r) and the layer's loss as one ledger record
// (gg_finish_mse_kernel), and a ReLU mask in the backward kernel's epilogue (gg_bwd_kernel's MASK flag).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <stdlib.h>

#include "fp16x3.hpp"

namespace maua {

constexpr int GG_T = 64;         // tile edge (channels)
constexpr int GG_K = 64;         // pixels per stage
constexpr int GG_RS = GG_K + 4;  // LDS row stride (floats): 16-byte aligned rows, conflict-free b128 reads (gram.hip)
constexpr int GG_RMAX = 8;       // most regions per call
constexpr int GG_MSPLIT = 64;    // most partial sums per (region, row) of the weighted row means
constexpr int GG_KMAX = 256;     // most slabs per (region, tile pair)

typedef float gg_f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// four consecutive values of a row whose end is `end` (elements beyond it read as 0); dword alignment is enough for the 16-byte load
__device__ __forceinline__ f32x4 gg_load4(const float* __restrict__ row, int64_t p, int64_t end) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p + 4 <= end) {
        v = *reinterpret_cast<const gg_f32x4u*>(row + p);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p + k < end) v[k] = row[p + k];
    }
    return v;
}

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

// One workgroup = one region x one upper-triangular 64x64 tile pair (ti <= tj) x one slice of HW; the four waves own a 32x32 block each
// (gram_partial_kernel's layout and MFMA pairing).  Slabs: partial[((r npairs + pair) ksplit + ks) 64 64].
__global__ void __launch_bounds__(256)
gg_partial_kernel(const float* __restrict__ f, const float* __restrict__ guides, const float* __restrict__ scale, const float* __restrict__ mean,
                  float* __restrict__ partial, int C, int64_t HW, int npairs, int ksplit, int64_t chunk) {
    __shared__ __attribute__((aligned(16))) float At[GG_T * GG_RS];
    __shared__ __attribute__((aligned(16))) float Bt[GG_T * GG_RS];
    const int reg = blockIdx.z;
    if (scale[reg] == 0.f) return;  // inactive region: the finishing kernel writes zeros without reading its slabs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i32 = lane & 31, half = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    int pair = blockIdx.x, ti = 0;
    const int ntile = (C + GG_T - 1) / GG_T;
    while (pair >= ntile - ti) {
        pair -= ntile - ti;
        ++ti;
    }
    const int tj = ti + pair;
    const bool diag = ti == tj;
    const int ks = blockIdx.y;
    const int64_t p_begin = (int64_t)ks * chunk;
    const int64_t p_end = min(HW, p_begin + chunk);
    const float* g = guides + (int64_t)reg * HW;
    const float* mu = mean ? mean + (int64_t)reg * C : nullptr;

    constexpr int NL = GG_T * GG_K / 4 / 256;  // 4 quads per tile per thread: rows tid / 16 + 16 q, pixels 4 (tid % 16) .. + 3
    const int r0 = tid >> 4, c4 = (tid & 15) * 4;
    float ma[NL], mb[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int rowa = ti * GG_T + r0 + 16 * q, rowb = tj * GG_T + r0 + 16 * q;
        ma[q] = (mu && rowa < C) ? mu[rowa] : 0.f;
        mb[q] = (mu && rowb < C) ? mu[rowb] : 0.f;
    }
    f32x4 ra[NL], rb[NL];
    // The guide quad of the stage after the one being loaded is requested a stage ahead, so the test below does not wait for memory.
    f32x4 gnext = p_begin < p_end ? gg_load4(g, p_begin + c4, p_end) : f32x4{0.f, 0.f, 0.f, 0.f};
    // -> true when the stage has a non-zero guide value; every wave's lanes 0 - 15 hold the stage's 64 guide values, so all four waves
    // of the workgroup decide alike and the barriers below stay matched
    auto load_stage = [&](int64_t p0) -> bool {
        const f32x4 gq = gnext;
        if (p0 + GG_K < p_end) gnext = gg_load4(g, p0 + GG_K + c4, p_end);
        const bool nz = gq[0] != 0.f || gq[1] != 0.f || gq[2] != 0.f || gq[3] != 0.f;
        if (__builtin_amdgcn_ballot_w64(nz) == 0ull) return false;
        const int64_t pp = p0 + c4;
        if (p0 + GG_K <= p_end && tj * GG_T + GG_T <= C) {  // workgroup-uniform: a whole stage of whole tiles, no per-load bounds
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                ra[q] = *reinterpret_cast<const gg_f32x4u*>(f + (int64_t)(ti * GG_T + r0 + 16 * q) * HW + pp);
                if (!diag) rb[q] = *reinterpret_cast<const gg_f32x4u*>(f + (int64_t)(tj * GG_T + r0 + 16 * q) * HW + pp);
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
            const int rowa = ti * GG_T + r0 + 16 * q, rowb = tj * GG_T + r0 + 16 * q;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            if (rowa < C) va = (gg_load4(f + (int64_t)rowa * HW, pp, p_end) - ma[q]) * gq;  // (cells beyond the slice: g = 0)
            if (!diag && rowb < C) vb = (gg_load4(f + (int64_t)rowb * HW, pp, p_end) - mb[q]) * gq;
            ra[q] = va;
            rb[q] = vb;
        }
        return true;
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            *reinterpret_cast<f32x4*>(At + (r0 + 16 * q) * GG_RS + c4) = ra[q];
            if (!diag) *reinterpret_cast<f32x4*>(Bt + (r0 + 16 * q) * GG_RS + c4) = rb[q];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bool skip = diag && wi == 1 && wj == 0;  // wave-uniform: the mirrored block of a diagonal tile

    if (p_begin < p_end) {
        bool act_next = load_stage(p_begin);
        for (int64_t p0 = p_begin; p0 < p_end; p0 += GG_K) {
            const bool act = act_next;  // workgroup-uniform
            if (act) {
                __syncthreads();  // previous stage fully consumed
                store_stage();
                __syncthreads();
            }
            if (p0 + GG_K < p_end) act_next = load_stage(p0 + GG_K);
            if (act && !skip) {
                const float* at = At + (wi * 32 + i32) * GG_RS + 4 * half;
                const float* bt = (diag ? At : Bt) + (wj * 32 + i32) * GG_RS + 4 * half;
#pragma unroll
                for (int q = 0; q < GG_K / 8; ++q) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(at + 8 * q);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(bt + 8 * q);
#pragma unroll
                    for (int cp = 0; cp < 4; ++cp) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cp], b[cp], acc, 0, 0, 0);
                }
            }
        }
    }
    float* out = partial + (((int64_t)reg * npairs + blockIdx.x) * ksplit + ks) * (GG_T * GG_T);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        out[row * GG_T + wj * 32 + i32] = acc[r];
    }
}

// grid (tile pairs, 16, R): every thread owns one element of the 64x64 tile, adds its slab values in index order (fp64), applies the
// region's scale and writes the element and its mirror; the lower triangle of a diagonal tile is read from the upper one.
__global__ void __launch_bounds__(256)
gg_finish_kernel(const float* __restrict__ partial, const float* __restrict__ scale, float* __restrict__ gram, int C, int npairs, int ksplit) {
    const int reg = blockIdx.z;
    int pair = blockIdx.x, ti = 0;
    const int ntile = (C + GG_T - 1) / GG_T;
    while (pair >= ntile - ti) {
        pair -= ntile - ti;
        ++ti;
    }
    const int tj = ti + pair;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int er = e / GG_T, ec = e % GG_T;
    const int src = (ti == tj && er > ec) ? ec * GG_T + er : e;
    const float sc = scale[reg];
    float s = 0.f;
    if (sc != 0.f) {
        const float* base = partial + ((int64_t)reg * npairs + blockIdx.x) * ksplit * (GG_T * GG_T) + src;
        double sd = 0.0;
        int k = 0;
        for (; k + 7 < ksplit; k += 8) {  // eight loads in flight, the additions in the order of a plain loop
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = base[(int64_t)(k + u) * (GG_T * GG_T)];
#pragma unroll
            for (int u = 0; u < 8; ++u) sd += (double)v[u];
        }
        for (; k < ksplit; ++k) sd += (double)base[(int64_t)k * (GG_T * GG_T)];
        s = (float)(sd * (double)sc);
    }
    const int gi = ti * GG_T + er, gj = tj * GG_T + ec;
    if (gi < C && gj < C) {
        float* gm = gram + (int64_t)reg * C * C;
        gm[(int64_t)gi * C + gj] = s;
        if (ti != tj) gm[(int64_t)gj * C + gi] = s;
    }
}

// gg_finish_kernel and the MSE against the regions' targets in one launch: grid (tile pairs, 16 / FQ, R), every thread owns FQ elements of
// the 64x64 tile (e = 256 (FQ blockIdx.y + u) + tid).  Each element's slab values are added in index order in fp64 exactly as
// gg_finish_kernel adds them (the same bits); the loads of the thread's FQ elements for eight slabs are requested together.
// D_r = grad_scale_r (G_r - T_r) is formed once per element of the upper triangle and written with its mirror (exactly symmetric whatever
// the target holds below its diagonal); exact zeros for a region with scale_r == 0 or grad_scale_r == 0.  The workgroup's share of
// loss_scale_r sum (G_r - T_r)^2 - off-diagonal tiles count twice - is one partial sum of the layer's ledger record (scale 1): R x pairs
// x 16 / FQ partial sums, a fixed order, no atomics.  The host takes the smallest FQ of 1, 2, 4 whose partial sums fit the record
// (gg_finish_split): FQ = 1 is gg_finish_kernel's grid - the serial chain of a thread is its slabs, so fewer, longer threads are slower
// where a layer has few tile pairs and many slabs - and FQ = 4 holds eight regions of 512 channels (8 x 36 x 4 sums).
constexpr int GG_FQ_MAX = 4;  // most elements per thread: 16 / 4 workgroups per (region, tile pair)
template <int FQ>
__global__ void __launch_bounds__(256)
gg_finish_mse_kernel(const float* __restrict__ partial, const float* __restrict__ scale, float* __restrict__ gram, int C, int npairs, int ksplit,
                     const float* __restrict__ target, const float* __restrict__ loss_scale, const float* __restrict__ grad_scale,
                     float* __restrict__ dmat, double* __restrict__ rec) {
    constexpr int GG_FQ = FQ;
    __shared__ double scratch[16];
    const int reg = blockIdx.z;
    int pair = blockIdx.x, ti = 0;
    const int ntile = (C + GG_T - 1) / GG_T;
    while (pair >= ntile - ti) {
        pair -= ntile - ti;
        ++ti;
    }
    const int tj = ti + pair;
    const float sc = scale[reg], ls = loss_scale[reg], gs = grad_scale[reg];
    int er[GG_FQ], ec[GG_FQ], src[GG_FQ];
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) {
        const int e = (blockIdx.y * GG_FQ + u) * 256 + threadIdx.x;
        er[u] = e / GG_T;
        ec[u] = e % GG_T;
        src[u] = (ti == tj && er[u] > ec[u]) ? ec[u] * GG_T + er[u] : e;
    }
    float s[GG_FQ];
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) s[u] = 0.f;
    if (sc != 0.f) {
        const float* base = partial + ((int64_t)reg * npairs + blockIdx.x) * ksplit * (GG_T * GG_T);
        double sd[GG_FQ];
#pragma unroll
        for (int u = 0; u < GG_FQ; ++u) sd[u] = 0.0;
        int k = 0;
        for (; k + 7 < ksplit; k += 8) {  // 8 GG_FQ loads in flight, each element's additions in the order of a plain loop
            float v[GG_FQ][8];
#pragma unroll
            for (int u = 0; u < GG_FQ; ++u)
#pragma unroll
                for (int w = 0; w < 8; ++w) v[u][w] = base[(int64_t)(k + w) * (GG_T * GG_T) + src[u]];
#pragma unroll
            for (int u = 0; u < GG_FQ; ++u)
#pragma unroll
                for (int w = 0; w < 8; ++w) sd[u] += (double)v[u][w];
        }
        for (; k < ksplit; ++k) {
            float v[GG_FQ];
#pragma unroll
            for (int u = 0; u < GG_FQ; ++u) v[u] = base[(int64_t)k * (GG_T * GG_T) + src[u]];
#pragma unroll
            for (int u = 0; u < GG_FQ; ++u) sd[u] += (double)v[u];
        }
#pragma unroll
        for (int u = 0; u < GG_FQ; ++u) s[u] = (float)(sd[u] * (double)sc);
    }
    const bool with_d = sc != 0.f && gs != 0.f;
    const int64_t mat = (int64_t)reg * C * C;
    double sq = 0.0;
#pragma unroll
    for (int u = 0; u < GG_FQ; ++u) {
        const int gi = ti * GG_T + er[u], gj = tj * GG_T + ec[u];
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
    sq = block_sum(sq, scratch);
    if (threadIdx.x == 0) {
        rec[2 + ((int64_t)reg * npairs + blockIdx.x) * gridDim.y + blockIdx.y] = sq * (double)ls;
        if (blockIdx.x == 0 && blockIdx.y == 0 && reg == 0) {
            rec[0] = (double)(gridDim.x * gridDim.y * gridDim.z);
            rec[1] = 1.0;
        }
    }
}

// Backward.  Workgroup = 64 output channels x 256 pixels, wave = 64 x 64 (2 x 2 accumulators), 32 input channels per LDS stage,
// double-buffered (80 KB); the stages run over (active region, channel block).
constexpr int GGB_KC = 32, GGB_PX = 256, GGB_CO = 64;

// MASK: the sums (and what they were accumulated into) are written as 0 where relu_mask[c][p] <= 0 (gram_bwd_kernel's pre-masked gradients).
template <bool ACC, bool MASK>
__global__ void __launch_bounds__(256)
gg_bwd_kernel(const float* __restrict__ d, const float* __restrict__ f, const float* __restrict__ guides, const float* __restrict__ coef,
              const float* __restrict__ mean, const float* __restrict__ relu_mask, float* __restrict__ gf, int R, int C, int64_t HW) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[32][256] + Wl[32][64])
    float* smem = smem_f32;
    constexpr int BUF = GGB_KC * GGB_PX + GGB_KC * GGB_CO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int64_t p0 = (int64_t)blockIdx.x * GGB_PX;
    const int co0 = blockIdx.y * GGB_CO;
    const int64_t pq = p0 + 4 * (tid & 63);  // this thread's pixel quad in every stage (each wave's 64 lanes cover the 256 pixels)

    // regions that take part: coef != 0 and a non-zero guide value among the workgroup's pixels (the same answer in every wave)
    unsigned active = 0;
    for (int r = 0; r < R; ++r) {
        const f32x4 gq = gg_load4(guides + (int64_t)r * HW, pq, HW);
        const bool nz = gq[0] != 0.f || gq[1] != 0.f || gq[2] != 0.f || gq[3] != 0.f;
        if (__builtin_amdgcn_ballot_w64(nz) != 0ull && coef[r] != 0.f) active |= 1u << r;
    }

    f32x4 rx[8], rw[2];
    auto load_stage = [&](int r, int k0) {
        const f32x4 gq = gg_load4(guides + (int64_t)r * HW, pq, HW);
        const float cf = coef[r];
        const f32x4 wq = gq * gq * cf;
        const float* dr = d + (int64_t)r * C * C;
        const float* mu = mean ? mean + (int64_t)r * C : nullptr;
        if (p0 + GGB_PX <= HW && k0 + GGB_KC <= C) {  // workgroup-uniform: 32 whole rows of 256 pixels, no per-load bounds
#pragma unroll
            for (int i = 0; i < 8; ++i) rx[i] = *reinterpret_cast<const gg_f32x4u*>(f + (int64_t)(k0 + (tid >> 6) + 4 * i) * HW + pq);
#pragma unroll
            for (int i = 0; i < 8; ++i) rx[i] = (rx[i] - (mu ? mu[k0 + (tid >> 6) + 4 * i] : 0.f)) * wq;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = k0 + (tid >> 6) + 4 * i;  // quad index tid + 256 i: 32 rows x 64 quads
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = (gg_load4(f + (int64_t)row * HW, pq, HW) - (mu ? mu[row] : 0.f)) * wq;  // (pixels beyond the plane: w = 0)
                rx[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i;  // 32 rows x 16 quads
            const int row = k0 + (e >> 4), q = e & 15;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < C) v = gg_load4(dr + (int64_t)row * C, co0 + 4 * q, C);
            rw[i] = v;
        }
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* wl = xl + GGB_KC * GGB_PX;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(xl + (tid + 256 * i) * 4) = rx[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(wl + (tid + 256 * i) * 4) = rw[i];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

    // the stage to load next: (region r, channel block k0); r == R: none left
    int r = 0, k0 = 0;
    while (r < R && !((active >> r) & 1u)) ++r;
    auto advance = [&]() {
        k0 += GGB_KC;
        if (k0 >= C) {
            k0 = 0;
            ++r;
            while (r < R && !((active >> r) & 1u)) ++r;
        }
    };
    if (r < R) {  // workgroup-uniform, as every branch on r below
        load_stage(r, k0);
        store_stage(0);
        advance();
        __syncthreads();
        int cur = 0;
        while (true) {
            const bool more = r < R;
            if (more) load_stage(r, k0);
            const float* xl = smem + cur * BUF;
            const float* wl = xl + GGB_KC * GGB_PX;
#pragma unroll
            for (int kp = 0; kp < GGB_KC / 2; ++kp) {
                const int kk = 2 * kp + half;
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = wl[kk * GGB_CO + t * 32 + j];
#pragma unroll
                for (int u = 0; u < 2; ++u) b[u] = xl[kk * GGB_PX + (wave * 2 + u) * 32 + j];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
            }
            if (more) {
                store_stage(cur ^ 1);
                advance();
            }
            __syncthreads();
            if (!more) break;
            cur ^= 1;
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t pix = p0 + (wave * 2 + u) * 32 + j;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // read-modify-write in two sweeps: all loads of the 16 registers first, then all stores (gram_bwd_kernel)
            float prev[16], mk[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = co0 + t * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                const bool ok = pix < HW && co < C;
                const int64_t o = ok ? (int64_t)co * HW + pix : 0;
                prev[q] = 0.f;
                mk[q] = 1.f;
                if constexpr (ACC) prev[q] = gf[o];
                if constexpr (MASK) mk[q] = relu_mask[o];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = co0 + t * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                float v = acc[t][u][q] + prev[q];
                if constexpr (MASK) v = mk[q] <= 0.f ? 0.f : v;
                if (pix < HW && co < C) gf[(int64_t)co * HW + pix] = v;
            }
        }
    }
}

// slabs per (region, tile pair) and their length in pixels: about 768 workgroups per region's matrix, slices of whole stages
static void gg_plan(int c, int64_t hw, int* npairs, int* ksplit, int64_t* chunk) {
    const int ntile = (c + GG_T - 1) / GG_T;
    *npairs = ntile * (ntile + 1) / 2;
    const int64_t stages = (hw + GG_K - 1) / GG_K;
    int64_t want = (768 + *npairs - 1) / *npairs;
    if (want > GG_KMAX) want = GG_KMAX;
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    const int64_t ch = ((hw + want - 1) / want + GG_K - 1) / GG_K * GG_K;
    *chunk = ch;
    *ksplit = (int)((hw + ch - 1) / ch);
}

// elements per thread of gg_finish_mse_kernel: the smallest of 1, 2, 4 for which regions x pairs x 16 / FQ partial sums fit one ledger record
// (0: not even GG_FQ_MAX does)
static int gg_finish_split(int regions, int64_t npairs) {
    for (int fq = 1; fq <= GG_FQ_MAX; fq *= 2)
        if ((int64_t)regions * npairs * (GG_T * GG_T / 256 / fq) <= LEDGER_MAX) return fq;
    return 0;
}

static bool gg_shape_ok(int regions, int c, int64_t hw) {
    return regions >= 1 && regions <= GG_RMAX && c >= 1 && c <= (1 << 16) && hw >= 1 && hw < (1ll << 30);
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_gram_guided_supported(int regions, int c, int64_t hw) { return gg_shape_ok(regions, c, hw) ? 1 : 0; }

size_t maua_gram_guided_workspace_bytes(int regions, int c, int64_t hw) {
    if (!gg_shape_ok(regions, c, hw)) return 0;
    int npairs, ksplit;
    int64_t chunk;
    gg_plan(c, hw, &npairs, &ksplit, &chunk);
    const size_t slabs = (size_t)regions * npairs * ksplit * GG_T * GG_T * sizeof(float);
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
    int npairs, ksplit;
    int64_t chunk;
    gg_plan(c, hw, &npairs, &ksplit, &chunk);
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
    hipLaunchKernelGGL(gg_partial_kernel, dim3(npairs, ksplit, regions), dim3(256), 0, s, f, guides, scale, center ? mean_out : nullptr,
                       (float*)workspace, c, hw, npairs, ksplit, chunk);
    int rc = check_launch("gg_partial_kernel");
    if (rc) return rc;
    if (mse) {
        const int fq = gg_finish_split(regions, npairs);
        auto finish = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(npairs, GG_T * GG_T / 256 / fq, regions), dim3(256), 0, s, (const float*)workspace, scale, gram, c, npairs,
                               ksplit, mse->target, mse->loss_scale, mse->grad_scale, mse->dmat, mse->rec);
        };
        if (fq == 1) finish(gg_finish_mse_kernel<1>);
        else if (fq == 2) finish(gg_finish_mse_kernel<2>);
        else finish(gg_finish_mse_kernel<4>);
        return check_launch("gg_finish_mse_kernel");
    }
    hipLaunchKernelGGL(gg_finish_kernel, dim3(npairs, GG_T * GG_T / 256, regions), dim3(256), 0, s, (const float*)workspace, scale, gram, c, npairs,
                       ksplit);
    return check_launch("gg_finish_kernel");
}

int maua_gram_guided_fwd(const float* f, const float* guides, const float* scale, const double* mass, float* gram, float* mean_out,
                         int regions, int c, int64_t hw, int center, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    return gg_forward("gram_guided_fwd", f, guides, scale, mass, gram, mean_out, regions, c, hw, center, workspace, workspace_bytes, nullptr, stream);
}

int maua_guided_gram_mse_ledger_supported(int regions, int c) {
    if (!gg_shape_ok(regions, c, 1)) return 0;
    const int64_t nt = (c + GG_T - 1) / GG_T;
    return gg_finish_split(regions, nt * (nt + 1) / 2) != 0 ? 1 : 0;
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
    constexpr size_t lds = 2ull * (GGB_KC * GGB_PX + GGB_KC * GGB_CO) * sizeof(float);
    const dim3 grid((unsigned)((hw + GGB_PX - 1) / GGB_PX), (unsigned)((c + GGB_CO - 1) / GGB_CO));
    auto launch = [&](auto kernel) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, d_sym, f, guides, coef, mean, relu_mask, gf, regions, c, hw);
    };
    if (relu_mask) {
        if (accumulate) launch(gg_bwd_kernel<true, true>);
        else launch(gg_bwd_kernel<false, true>);
    } else {
        if (accumulate) launch(gg_bwd_kernel<true, false>);
        else launch(gg_bwd_kernel<false, false>);
    }
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
