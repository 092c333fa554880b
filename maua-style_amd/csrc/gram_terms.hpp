// The tile engine shared by the shifted, mirrored and guided Gram terms (gram_shift.hip, gram_flip.hip, gram_guided.hip; DESIGN.md section
// 11).  Each file keeps its operand loaders, its pair enumeration and its kernel entry points; the parts below exist once.
// Include this header only from a file that carries the `// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops` line: every
// kernel built from it issues MFMAs (build_native.py says why packed fp32 is off beside them).
//
// Forward.  A term (a shift, a mirror, a region) is the third grid dimension.  One workgroup = one term x one pair (ti, tj) of 64-channel
// tiles x one slice of the plane.  A stage is 64 pixels: two operand tiles At (rows of G), Bt (columns of G) of 64 x 64 floats in LDS, row
// stride 68 (16-byte aligned rows, conflict-free b128 reads); thread tid loads the rows tid / 16 + 16 q, pixels 4 (tid % 16) .. + 3.  The
// four waves own a 32 x 32 block each (wi = wave / 2, wj = wave % 2), fp32 MFMA 32x32x2.
// Slabs: partial[((term npairs + pair) ksplit + ks) 64 64], one 64 x 64 fp32 tile per workgroup.  The slicing of the plane (gt_plan) is a
// function of (C, H W) alone, so a term has the same bits alone or among others.  A finishing kernel adds an element's ksplit slab values
// in index order in fp64 (gt_fold) and applies the term's factor: deterministic, no float atomics.
// Ledger record of an _mse finishing launch on a grid (pairs, 16 / FQ, terms): {number of partial sums, 1, sums ...} with the sum of
// workgroup (x, y, term) at 2 + (term pairs + x) gridDim.y + y.
// Backward.  One workgroup = 64 output channels x 256 pixels, wave = 64 x 64 (2 x 2 accumulators); a stage is 32 input channels,
// Xl[32][256] + Wl[32][64] floats, double-buffered (80 KB of dynamic LDS).  The stages run over (run, channel block); a family's runs are
// its terms (shift: two per term) and a run whose bit in `active` is clear is left out.
#pragma once
#include <stdlib.h>

#include "fp16x3.hpp"

namespace maua {

constexpr int GT_T = 64;         // tile edge (channels)
constexpr int GT_K = 64;         // pixels per stage
constexpr int GT_RS = GT_K + 4;  // LDS row stride (floats)
constexpr int GT_FQ_MAX = 4;     // most elements per thread of an _mse finishing kernel: 16 / 4 workgroups per (term, tile pair)
constexpr int GTB_KC = 32, GTB_PX = 256, GTB_CO = 64;
constexpr size_t GTB_LDS = 2ull * (GTB_KC * GTB_PX + GTB_KC * GTB_CO) * sizeof(float);

typedef float gt_f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // dword alignment is enough for the 16-byte load

// row[p + k] - mu for the elements k of the mask, 0 for the others; only the mask's addresses are formed.  I: the family's pixel index type.
template <class I>
__device__ __forceinline__ f32x4 gt_load4(const float* __restrict__ row, I p, unsigned m, float mu) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m == 15u) {
        v = *reinterpret_cast<const gt_f32x4u*>(row + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] -= mu;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((m >> k) & 1u) v[k] = row[p + k] - mu;
    }
    return v;
}

// four consecutive values of a row whose end is `end` (elements beyond it read as 0)
__device__ __forceinline__ f32x4 gt_load4_end(const float* __restrict__ row, int64_t p, int64_t end) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p + 4 <= end) {
        v = *reinterpret_cast<const gt_f32x4u*>(row + p);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p + k < end) v[k] = row[p + k];
    }
    return v;
}

// the b-th pair (ti <= tj) of ntile tiles, rows first: (0,0) (0,1) .. (0,n-1) (1,1) ..
__device__ __forceinline__ void gt_pair_upper(int b, int ntile, int* ti, int* tj) {
    int i = 0;
    while (b >= ntile - i) {
        b -= ntile - i;
        ++i;
    }
    *ti = i;
    *tj = i + b;
}

__device__ __forceinline__ f32x16 gt_zero16() {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    return acc;
}

// this wave's 32 x 32 block of one staged pair of tiles (Bt may be At)
__device__ __forceinline__ void gt_mma_stage(const float* At, const float* Bt, f32x16& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i32 = lane & 31, half = lane >> 5;
    const float* at = At + ((wave >> 1) * 32 + i32) * GT_RS + 4 * half;
    const float* bt = Bt + ((wave & 1) * 32 + i32) * GT_RS + 4 * half;
#pragma unroll
    for (int q = 0; q < GT_K / 8; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(at + 8 * q);
        const f32x4 b = *reinterpret_cast<const f32x4*>(bt + 8 * q);
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cp], b[cp], acc, 0, 0, 0);
    }
}

// this wave's accumulator into the workgroup's slab
__device__ __forceinline__ void gt_store_slab(float* __restrict__ partial, int term, int npairs, int ksplit, const f32x16& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i32 = lane & 31, half = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    float* out = partial + (((int64_t)term * npairs + blockIdx.x) * ksplit + blockIdx.y) * (GT_T * GT_T);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        out[row * GT_T + wj * 32 + i32] = acc[r];
    }
}

// the slabs of the workgroup's (term, tile pair)
__device__ __forceinline__ const float* gt_slabs(const float* __restrict__ partial, int term, int npairs, int ksplit) {
    return partial + ((int64_t)term * npairs + blockIdx.x) * ksplit * (GT_T * GT_T);
}

// sd[u] = the slab values of tile element e[u], added in slab index order in fp64: the loads of N slabs for the thread's FQ elements are
// requested together, each element's additions are those of a plain loop.
template <int N, int FQ>
__device__ __forceinline__ void gt_fold(const float* __restrict__ base, const int (&e)[FQ], int ksplit, double (&sd)[FQ]) {
#pragma unroll
    for (int u = 0; u < FQ; ++u) sd[u] = 0.0;
    int k = 0;
    for (; k + N - 1 < ksplit; k += N) {
        float v[FQ][N];
#pragma unroll
        for (int u = 0; u < FQ; ++u)
#pragma unroll
            for (int w = 0; w < N; ++w) v[u][w] = base[(int64_t)(k + w) * (GT_T * GT_T) + e[u]];
#pragma unroll
        for (int u = 0; u < FQ; ++u)
#pragma unroll
            for (int w = 0; w < N; ++w) sd[u] += (double)v[u][w];
    }
    for (; k < ksplit; ++k) {
        float v[FQ];
#pragma unroll
        for (int u = 0; u < FQ; ++u) v[u] = base[(int64_t)k * (GT_T * GT_T) + e[u]];
#pragma unroll
        for (int u = 0; u < FQ; ++u) sd[u] += (double)v[u];
    }
}

// the workgroup's entry of the ledger record: `sq` is this thread's share, `weigh` the term's loss scale applied to the workgroup's sum
template <class Weigh>
__device__ __forceinline__ void gt_ledger_put(double sq, int term, int npairs, double* __restrict__ rec, const Weigh& weigh) {
    __shared__ double scratch[16];
    sq = block_sum(sq, scratch);
    if (threadIdx.x == 0) {
        rec[2 + ((int64_t)term * npairs + blockIdx.x) * gridDim.y + blockIdx.y] = weigh(sq);
        if (blockIdx.x == 0 && blockIdx.y == 0 && term == 0) {
            rec[0] = (double)(gridDim.x * gridDim.y * gridDim.z);
            rec[1] = 1.0;
        }
    }
}

// The backward pipeline and epilogue.  load_stage(run, k0) fetches the stage of channel block k0 of a run into registers, store_stage(buf)
// writes those registers to LDS buffer buf (Xl at smem + buf BUF, Wl behind it); every branch on the run is workgroup-uniform.
// ACC: gx += the sums.  MASK: the sums (and what they were accumulated into) are written as 0 where relu_mask[c][p] <= 0.
template <bool ACC, bool MASK, class I, class Load, class Store>
__device__ __forceinline__ void gt_bwd_run(const float* smem, unsigned active, int nruns, int C, I HW, I p0, int co0,
                                           const float* __restrict__ relu_mask, float* __restrict__ gx, const Load& load_stage,
                                           const Store& store_stage) {
    constexpr int BUF = GTB_KC * GTB_PX + GTB_KC * GTB_CO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = gt_zero16();

    // the stage to load next: (run st, channel block k0); st == nruns: none left
    int st = 0, k0 = 0;
    while (st < nruns && !((active >> st) & 1u)) ++st;
    auto advance = [&]() {
        k0 += GTB_KC;
        if (k0 >= C) {
            k0 = 0;
            ++st;
            while (st < nruns && !((active >> st) & 1u)) ++st;
        }
    };
    if (st < nruns) {
        load_stage(st, k0);
        store_stage(0);
        advance();
        __syncthreads();
        int cur = 0;
        while (true) {
            const bool more = st < nruns;
            if (more) load_stage(st, k0);
            const float* xl = smem + cur * BUF;
            const float* wl = xl + GTB_KC * GTB_PX;
#pragma unroll
            for (int kp = 0; kp < GTB_KC / 2; ++kp) {
                const int kk = 2 * kp + half;
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = wl[kk * GTB_CO + t * 32 + j];
#pragma unroll
                for (int u = 0; u < 2; ++u) b[u] = xl[kk * GTB_PX + (wave * 2 + u) * 32 + j];
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
        const I pix = p0 + (wave * 2 + u) * 32 + j;
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
                if constexpr (ACC) prev[q] = gx[o];
                if constexpr (MASK) mk[q] = relu_mask[o];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = co0 + t * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                float v = acc[t][u][q] + prev[q];
                if constexpr (MASK) v = mk[q] <= 0.f ? 0.f : v;
                if (pix < HW && co < C) gx[(int64_t)co * HW + pix] = v;
            }
        }
    }
}

// Host side.

static bool gt_shape_ok(int terms, int most, int c, int64_t hw) {
    return terms >= 1 && terms <= most && c >= 1 && c <= (1 << 16) && hw >= 1 && hw < (1ll << 30);
}

static int64_t gt_pairs(int c, bool all_pairs) {
    const int64_t ntile = (c + GT_T - 1) / GT_T;
    return all_pairs ? ntile * ntile : ntile * (ntile + 1) / 2;
}

// slabs per (term, tile pair) and their length in pixels: about 768 workgroups per term's matrix, at most kmax slabs, slices of whole
// stages - a function of (C, H W) alone
struct GtPlan {
    int npairs, ksplit;
    int64_t chunk;
    size_t slab_bytes(int terms) const { return (size_t)terms * npairs * ksplit * GT_T * GT_T * sizeof(float); }
};
static GtPlan gt_plan(int c, int64_t hw, bool all_pairs, int kmax) {
    GtPlan p;
    p.npairs = (int)gt_pairs(c, all_pairs);
    const int64_t stages = (hw + GT_K - 1) / GT_K;
    int64_t want = (768 + p.npairs - 1) / p.npairs;
    if (want > kmax) want = kmax;
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    p.chunk = ((hw + want - 1) / want + GT_K - 1) / GT_K * GT_K;
    p.ksplit = (int)((hw + p.chunk - 1) / p.chunk);
    return p;
}

// elements per thread of an _mse finishing kernel: the smallest of 1, 2, 4 for which terms x pairs x 16 / FQ partial sums fit one ledger
// record (0: not even GT_FQ_MAX does)
static int gt_finish_split(int terms, int64_t npairs) {
    for (int fq = 1; fq <= GT_FQ_MAX; fq *= 2)
        if ((int64_t)terms * npairs * (GT_T * GT_T / 256 / fq) <= LEDGER_MAX) return fq;
    return 0;
}

// the _mse finishing launch: kernel<FQ> on the grid (pairs, 16 / FQ, terms)
template <class Kn, class... Args>
static void gt_launch_finish_mse(Kn k1, Kn k2, Kn k4, int terms, const GtPlan& p, hipStream_t s, Args... args) {
    const int fq = gt_finish_split(terms, p.npairs);
    const Kn kernel = fq == 1 ? k1 : fq == 2 ? k2 : k4;
    hipLaunchKernelGGL(kernel, dim3(p.npairs, GT_T * GT_T / 256 / fq, terms), dim3(256), 0, s, args...);
}

// the backward launch: kernel<ACC, MASK> given as <0,0> <1,0> <0,1> <1,1>
template <class Kn, class... Args>
static void gt_launch_bwd(Kn plain, Kn acc, Kn masked, Kn acc_masked, bool accumulate, bool mask, int c, int64_t hw, hipStream_t s, Args... args) {
    const Kn kernel = mask ? (accumulate ? acc_masked : masked) : (accumulate ? acc : plain);
    const dim3 grid((unsigned)((hw + GTB_PX - 1) / GTB_PX), (unsigned)((c + GTB_CO - 1) / GTB_CO));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GTB_LDS);
    hipLaunchKernelGGL(kernel, grid, dim3(256), GTB_LDS, s, args...);
}

}  // namespace maua
