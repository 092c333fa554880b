// The feature-histogram device code shared by feat_hist.hip and swd.hip (DESIGN.md sections 15 and 17): the launch plan, the sweep over a
// chunk, the range fold, the pinned bin arithmetic, the matched value, and the count, scan, residual and finish kernels.  The kernels have
// internal linkage: each file that includes this header launches its own copies.
#pragma once
#include <stdlib.h>

#include "common.hpp"

namespace maua {

constexpr int FH_THREADS = 256;
constexpr int FH_GRAIN = 4 * FH_THREADS;  // chunk granularity (elements): one quad per thread
constexpr int FH_WGS = 2048;              // workgroups a streaming launch aims at: 8 per CU
constexpr int FH_UNROLL = 4;              // quads a thread requests before it uses the first
constexpr int FH_BINS_MIN = 16, FH_BINS_MAX = 1024;
constexpr int FH_KNOTS_MIN = 2, FH_KNOTS_MAX = 4096;

typedef float fh_f32x4 __attribute__((ext_vector_type(4)));

static bool fh_shape_ok(int c, int h, int w, int bins, int knots) {
    return c >= 1 && c <= (1 << 16) && h >= 1 && w >= 1 && (int64_t)h * w < (1ll << 30) && bins >= FH_BINS_MIN && bins <= FH_BINS_MAX &&
           knots >= FH_KNOTS_MIN && knots <= FH_KNOTS_MAX;
}

// pieces of a channel's plane and their length: about FH_WGS workgroups over all channels, pieces of whole grains
static void fh_plan(int c, int64_t n, int* chunks, int* chunk) {
    int64_t want = (FH_WGS + c - 1) / c;
    const int64_t grains = (n + FH_GRAIN - 1) / FH_GRAIN;
    if (want > grains) want = grains;
    if (want < 1) want = 1;
    const int64_t ch = ((n + want - 1) / want + FH_GRAIN - 1) / FH_GRAIN * FH_GRAIN;  // <= n + 2 FH_GRAIN < 2^31
    *chunk = (int)ch;
    *chunks = (int)((n + ch - 1) / ch);
}

// state: per channel bins + 3 words - lo, hi (fp32), cum[0 .. bins] (int32)
__device__ __forceinline__ int* fh_state(int* state, int c, int bins) { return state + (int64_t)c * (bins + 3); }
__device__ __forceinline__ const int* fh_state(const int* state, int c, int bins) { return state + (int64_t)c * (bins + 3); }

// The elements [0, n) of a chunk at src, each once: op1(i, v) for the scalar head and tail, op4(i, v) for the quad at i .. i + 3.  `vec`
// false: every element goes through op1.
template <class Op1, class Op4>
__device__ __forceinline__ void fh_sweep(const float* __restrict__ src, int n, bool vec, Op1&& op1, Op4&& op4) {
    const int tid = threadIdx.x;
    int head = n;
    if (vec) head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) >> 2));
    const int nq = (n - head) >> 2;
    const int tail = head + 4 * nq;
    for (int i = tid; i < head; i += FH_THREADS) op1(i, src[i]);
    const fh_f32x4* __restrict__ q4 = reinterpret_cast<const fh_f32x4*>(src + head);
    for (int q0 = tid; q0 < nq; q0 += FH_UNROLL * FH_THREADS) {
        fh_f32x4 v[FH_UNROLL];
#pragma unroll
        for (int u = 0; u < FH_UNROLL; ++u)
            if (q0 + u * FH_THREADS < nq) v[u] = q4[q0 + u * FH_THREADS];
#pragma unroll
        for (int u = 0; u < FH_UNROLL; ++u)
            if (q0 + u * FH_THREADS < nq) op4(head + 4 * (q0 + u * FH_THREADS), v[u]);
    }
    if (tid < n - tail) op1(tail + tid, src[tail + tid]);  // fewer than four
}

// minimum and maximum over the workgroup, in every thread; scratch: 8 floats
__device__ __forceinline__ void fh_block_minmax(float* lo, float* hi, float* scratch) {
    float a = *lo, b = *hi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a = fminf(a, __shfl_xor(a, off, 64));
        b = fmaxf(b, __shfl_xor(b, off, 64));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // scratch may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) {
        scratch[wave] = a;
        scratch[4 + wave] = b;
    }
    __syncthreads();
    a = fminf(fminf(scratch[0], scratch[1]), fminf(scratch[2], scratch[3]));
    b = fmaxf(fmaxf(scratch[4], scratch[5]), fmaxf(scratch[6], scratch[7]));
    *lo = a;
    *hi = b;
}

// the channel's range from its slabs minmax[c][slabs][2]: one per chunk of fh_range_kernel, or one per span of swd_project_kernel
__device__ __forceinline__ void fh_fold_range(const float* __restrict__ minmax, int c, int slabs, float* lo, float* hi, float* scratch) {
    float a = INFINITY, b = -INFINITY;
    const float* mm = minmax + (int64_t)c * slabs * 2;
    for (int i = threadIdx.x; i < slabs; i += FH_THREADS) {
        a = fminf(a, mm[2 * i]);
        b = fmaxf(b, mm[2 * i + 1]);
    }
    fh_block_minmax(&a, &b, scratch);
    *lo = a;
    *hi = b;
}

__device__ __forceinline__ float fh_inv(float lo, float hi, int bins) {
    return hi == lo ? 0.f : (float)((double)bins / ((double)hi - (double)lo));
}

// the decision: bin and position inside it.  (The lower clamp changes nothing for lo <= v <= hi; it keeps a NaN out of the LDS index.)
__device__ __forceinline__ void fh_bin(float v, float lo, float inv, int bins, int* b, float* frac) {
    const float t = __fmul_rn(__fsub_rn(v, lo), inv);
    const int bb = max(0, min(bins - 1, (int)t));
    *b = bb;
    *frac = fminf(1.0f, __fsub_rn(t, (float)bb));
}

// the matched value of v; cum[0 .. bins] and tab[0 .. knots) in LDS
__device__ __forceinline__ float fh_match(float v, float lo, float inv, int bins, int knots, float nf, const int* cum, const float* tab) {
    int b;
    float frac;
    fh_bin(v, lo, inv, bins, &b, &frac);
    const int c0 = cum[b], c1 = cum[b + 1];
    const float q = ((float)c0 + frac * (float)(c1 - c0)) / nf;
    const float p = fminf(fmaxf(q * (float)knots - 0.5f, 0.f), (float)(knots - 1));
    const int i0 = max(0, min(knots - 2, (int)p));
    const float t0 = tab[i0];
    return t0 + (p - (float)i0) * (tab[i0 + 1] - t0);
}

static __global__ void __launch_bounds__(FH_THREADS)
fh_range_kernel(const float* __restrict__ f, int* __restrict__ state, float* __restrict__ minmax, int N, int chunks, int chunk, int bins) {
    __shared__ float scratch[8];
    const int c = blockIdx.x / chunks, ks = blockIdx.x - c * chunks;
    const int p0 = ks * chunk;  // < N
    const int n = min(chunk, N - p0);
    float lo = INFINITY, hi = -INFINITY;
    auto op1 = [&](int, float v) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    };
    auto op4 = [&](int, fh_f32x4 v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) op1(0, v[k]);
    };
    fh_sweep(f + (int64_t)c * N + p0, n, true, op1, op4);
    fh_block_minmax(&lo, &hi, scratch);
    if (threadIdx.x == 0) {
        float* mm = minmax + ((int64_t)c * chunks + ks) * 2;
        mm[0] = lo;
        mm[1] = hi;
    }
    if (ks == 0) {
        int* cum = fh_state(state, c, bins) + 2;
        for (int b = threadIdx.x; b <= bins; b += FH_THREADS) cum[b] = 0;
    }
}

static __global__ void __launch_bounds__(FH_THREADS)
fh_count_kernel(const float* __restrict__ f, int* __restrict__ state, const float* __restrict__ minmax, int N, int chunks, int chunk, int bins,
                int slabs) {
    __shared__ float scratch[8];
    __shared__ int hist[FH_BINS_MAX];
    const int c = blockIdx.x / chunks, ks = blockIdx.x - c * chunks;
    const int p0 = ks * chunk;
    const int n = min(chunk, N - p0);
    for (int b = threadIdx.x; b < bins; b += FH_THREADS) hist[b] = 0;
    float lo, hi;
    fh_fold_range(minmax, c, slabs, &lo, &hi, scratch);  // (its barriers also publish the zeroed histogram)
    const float inv = fh_inv(lo, hi, bins);
    auto op1 = [&](int, float v) {
        int b;
        float frac;
        fh_bin(v, lo, inv, bins, &b, &frac);
        const unsigned long long zero = __ballot(b == 0);  // the lanes that are here and in bin 0: one add for all of them
        if (b != 0) atomicAdd(&hist[b], 1);
        else if ((int)(threadIdx.x & 63) == __ffsll((long long)zero) - 1) atomicAdd(&hist[0], __popcll(zero));
    };
    auto op4 = [&](int, fh_f32x4 v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) op1(0, v[k]);
    };
    fh_sweep(f + (int64_t)c * N + p0, n, true, op1, op4);
    __syncthreads();
    int* cnt = fh_state(state, c, bins) + 2;
    for (int b = threadIdx.x; b < bins; b += FH_THREADS) {
        const int v = hist[b];
        if (v) atomicAdd(&cnt[b], v);
    }
}

// grid C: the counters of a channel become their exclusive prefix sum, in place
static __global__ void __launch_bounds__(FH_THREADS)
fh_scan_kernel(int* __restrict__ state, const float* __restrict__ minmax, int slabs, int bins) {
    __shared__ float scratch[8];
    __shared__ int part[FH_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x;
    int* st = fh_state(state, c, bins);
    int* cum = st + 2;
    constexpr int PER = FH_BINS_MAX / FH_THREADS;  // consecutive bins per thread
    int v[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int b = tid * PER + k;
        v[k] = b < bins ? cum[b] : 0;
        sum += v[k];
    }
    part[tid] = sum;
    __syncthreads();  // every counter is in registers from here on
    for (int off = 1; off < FH_THREADS; off <<= 1) {
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int run = part[tid] - sum;  // exclusive
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int b = tid * PER + k;
        if (b < bins) cum[b] = run;
        run += v[k];
    }
    if (tid == FH_THREADS - 1) cum[bins] = part[tid];  // = N
    float lo, hi;
    fh_fold_range(minmax, c, slabs, &lo, &hi, scratch);
    if (tid == 0) {
        reinterpret_cast<float*>(st)[0] = lo;
        reinterpret_cast<float*>(st)[1] = hi;
    }
}

// T_c and cum_c into LDS, lo and inv from the state
__device__ __forceinline__ void fh_stage(const float* __restrict__ table, const int* __restrict__ state, int c, int bins, int knots, float* tab,
                                         int* cum, float* lo, float* inv) {
    const int* st = fh_state(state, c, bins);
    const float* tc = table + (int64_t)c * knots;
    for (int k = threadIdx.x; k < knots; k += FH_THREADS) tab[k] = tc[k];
    for (int b = threadIdx.x; b <= bins; b += FH_THREADS) cum[b] = st[2 + b];
    const float l = reinterpret_cast<const float*>(st)[0], h = reinterpret_cast<const float*>(st)[1];
    *lo = l;
    *inv = fh_inv(l, h, bins);
    __syncthreads();
}

static __global__ void __launch_bounds__(FH_THREADS)
fh_resid_kernel(const float* __restrict__ f, const float* __restrict__ table, const int* __restrict__ state, double* __restrict__ partial, int N,
                int chunks, int chunk, int bins, int knots) {
    __shared__ float tab[FH_KNOTS_MAX];
    __shared__ int cum[FH_BINS_MAX + 1];
    __shared__ double scratch[16];
    const int c = blockIdx.x / chunks, ks = blockIdx.x - c * chunks;
    const int p0 = ks * chunk;
    const int n = min(chunk, N - p0);
    float lo, inv;
    fh_stage(table, state, c, bins, knots, tab, cum, &lo, &inv);
    const float nf = (float)N;
    double acc = 0.0;
    auto op1 = [&](int, float v) {
        const float d = v - fh_match(v, lo, inv, bins, knots, nf, cum, tab);
        acc += (double)d * (double)d;
    };
    auto op4 = [&](int, fh_f32x4 v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) op1(0, v[k]);
    };
    fh_sweep(f + (int64_t)c * N + p0, n, true, op1, op4);
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[(int64_t)c * chunks + ks] = acc;
}

// one workgroup: thread t adds the partial sums t, t + 256, ... in order, then a tree of fixed shape
static __global__ void __launch_bounds__(FH_THREADS)
fh_finish_kernel(const double* __restrict__ partial, int n, double scale, float* __restrict__ loss) {
    __shared__ double scratch[16];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += FH_THREADS) v += partial[i];
    v = block_sum(v, scratch);
    if (threadIdx.x == 0) loss[0] = (float)(v * scale);
}

}  // namespace maua
