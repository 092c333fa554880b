// Sliced Wasserstein style loss (Heitz, Vanhoey, Chambon & Belcour 2021): the feature vectors of a style layer's activation F[C][N] (N = H W)
// are projected onto D directions V[D][C] (rows of unit length), and along every direction the projected values are matched to the style's
// projected distribution by monotone rearrangement - which is the feature-histogram match of DESIGN.md section 15 applied to P = V F with D in
// the place of C:
//     P = V F                                                     fp32 matrix cores, fixed summation order
//     lo, hi, bin, counts, cum, matched value R of P              section 15, unchanged (feat_hist.hpp)
//     s = sum (P - R)^2 / (D N),   ds/dF = 2 / (D N) V^T (P - R)   R is a constant in the derivative
// Launch plan.
//   forward   swd_project_kernel  P = V F, a (D x C) by (C x N) product on v_mfma_f32_32x32x2f32.  A workgroup owns 32 TA rows of P (TA = 1, 2
//                                 or 4: sw_ta) and a span of consecutive tiles of 256 pixels (a wave 64 of them); a stage is 16 values of
//                                 K for the tile: 16 x 256 of F and 16 x 32 TA of V through double-buffered LDS, read back as in
//                                 mrf_match_kernel.  K runs in stage order, inside a stage in pairs: the same inputs give the same bits.
//                                 A row past D, a pixel past N or a k past C is decided from indices before any address is formed and
//                                 staged as 0.  Epilogue: P is stored and, with a state, the (min, max) of the workgroup's piece of every
//                                 row goes to a slab in the workspace - lanes fold their 16 rows by a halving butterfly (16 + 16 shuffles
//                                 per 32 rows), waves through LDS, tiles of the span in LDS - and the workgroups of span 0 zero the rows'
//                                 bins + 1 counters: the range pass over P does not exist.
//             fh_count_kernel, fh_scan_kernel   section 15's, on P; they fold the projection's slabs
//             swd_resid_kernel    fh_resid_kernel that also writes G = P - R over P: after the forward call the buffer holds G
//             fh_finish_kernel    section 15's
//   backward  swd_back_kernel     gF (+)= coef upstream V^T G: the same product with V^T [C][D] (made once by the caller) in the place of V
//                                 and G in the place of F; the epilogue scales and writes, or reads, adds and writes
// No float atomics, losses through fixed-order fp64 sums.  No packed fp32 instructions beside the MFMAs (build_native._file_flags).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include "feat_hist.hpp"
#include "fp16x3.hpp"

namespace maua {

constexpr int SW_KC = 16;     // values of K per stage
constexpr int SW_NT = 256;    // pixels per tile
constexpr int SW_WGS = 1024;  // workgroups a product aims at: 4 per CU
constexpr int SW_FILL = 512;  // workgroups that fill the chip: two per CU
constexpr int SW_SMALL = 64;  // fewer 32-row workgroups than this: the product is one partial wave of work whatever its tile
constexpr int SW_CMAX = 4096;

static bool sw_shape_ok(int c, int d, int h, int w) {
    return c >= 1 && c <= SW_CMAX && d >= 1 && d <= SW_CMAX && h >= 1 && w >= 1 && (int64_t)h * w < (1ll << 30);
}

// 32-row blocks of a workgroup's tile (TA).  For a product too small to fill the chip, by its rows alone: 1 up to 32 rows, 2 up to 64, else 4.
// Else the largest of these that still gives SW_FILL workgroups, 1 if none does (512 rows over 4096 pixels: 256 workgroups of 32 rows
// instead of 64 of 128).  A function of (m, n) alone.
static int sw_ta(int m, int64_t n) {
    const int64_t nt = (n + SW_NT - 1) / SW_NT;
    const int by_rows = m <= 32 ? 1 : m <= 64 ? 2 : 4;
    if ((int64_t)((m + 31) / 32) * nt < SW_SMALL) return by_rows;
    for (int ta = by_rows; ta > 1; ta >>= 1)
        if ((int64_t)((m + 32 * ta - 1) / (32 * ta)) * nt >= SW_FILL) return ta;
    return 1;
}

// A product with m output rows over n pixels: pixel tiles, tiles per workgroup (`span`) and workgroups along the pixels (`slabs`) - about
// SW_WGS workgroups, a function of (m, n) alone
static void sw_plan(int m, int64_t n, int* ntiles, int* span, int* slabs) {
    const int mt = 32 * sw_ta(m, n);
    const int mtiles = (m + mt - 1) / mt;
    const int nt = (int)((n + SW_NT - 1) / SW_NT);
    int want = SW_WGS / mtiles;
    if (want < 1) want = 1;
    const int sp = (nt + want - 1) / want;
    *ntiles = nt;
    *span = sp;
    *slabs = (nt + sp - 1) / sp;
}

// One step of the halving butterfly: of 2 H values a lane keeps the half its bit names and folds the partner's into it.
template <int H>
__device__ __forceinline__ void sw_fold(float* mn, float* mx, bool bit, int mask) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float kn = bit ? mn[i + H] : mn[i], sn = bit ? mn[i] : mn[i + H];
        const float kx = bit ? mx[i + H] : mx[i], sx = bit ? mx[i] : mx[i + H];
        mn[i] = fminf(kn, __shfl_xor(sn, mask, 64));
        mx[i] = fmaxf(kx, __shfl_xor(sx, mask, 64));
    }
}

// out[M][N] = a[M][K] x[K][N].  MODE 0: stored; 1: stored, slabs and counters (the projection with a state); 2: scale x product written;
// 3: scale x product added.  grid (slabs, row tiles).
template <int TA, int MODE>
__device__ __forceinline__ void sw_product(const float* __restrict__ a, const float* __restrict__ x, float* __restrict__ out, int M, int K, int N,
                                           int span, int ntiles, float* __restrict__ minmax, int* __restrict__ state, int bins, float scale) {
    constexpr int MT = 32 * TA, LDA = MT + 1, AW = SW_KC * MT / 256, BUF = SW_KC * SW_NT + SW_KC * LDA;
    constexpr bool RANGE = MODE == 1;
    __shared__ __attribute__((aligned(16))) float smem[2 * BUF];  // 2 x (Xl[SW_KC][256] + Al[SW_KC][LDA])
    __shared__ float red[RANGE ? 2 * 4 * MT : 1];                 // (min | max) of a wave's 64 pixels per row
    __shared__ float run[RANGE ? 2 * MT : 1];                     // (min | max) of the span so far per row, owned by thread `row`
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.y * MT;
    const int t0 = blockIdx.x * span;  // < ntiles (sw_plan)
    const int ntile = min(ntiles, t0 + span) - t0;
    const int nblk = (K + SW_KC - 1) / SW_KC;
    const int total = ntile * nblk;

    if constexpr (RANGE) {
        if (blockIdx.x == 0) {
            const int per = bins + 1;
            for (int i = tid; i < MT * per; i += 256) {
                const int row = m0 + i / per;
                if (row < M) fh_state(state, row, bins)[2 + i % per] = 0;
            }
        }
    }

    const int ak = tid & (SW_KC - 1), arow = tid / SW_KC;  // this thread's k of a stage of `a`, and its first row
    int lt = 0, cb = 0;                                     // the stage to load next
    float rx[SW_KC], ra[AW];
    auto load_stage = [&]() {
        const int n = (t0 + lt) * SW_NT + tid;  // < 2^30 + 256
        const int k0 = cb * SW_KC;
#pragma unroll
        for (int i = 0; i < SW_KC; ++i) {
            const int k = k0 + i;
            rx[i] = (n < N && k < K) ? x[(int64_t)k * N + n] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < AW; ++i) {
            const int row = m0 + arow + (256 / SW_KC) * i;
            ra[i] = (row < M && k0 + ak < K) ? a[(int64_t)row * K + k0 + ak] : 0.f;
        }
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* al = xl + SW_KC * SW_NT;
#pragma unroll
        for (int i = 0; i < SW_KC; ++i) xl[i * SW_NT + tid] = rx[i];
#pragma unroll
        for (int i = 0; i < AW; ++i) al[ak * LDA + arow + (256 / SW_KC) * i] = ra[i];
    };
    auto advance = [&]() {
        if (++cb == nblk) {
            cb = 0;
            ++lt;
        }
    };

    f32x16 acc[TA][2];
    auto clear = [&]() {
#pragma unroll
        for (int t = 0; t < TA; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    };
    clear();

    load_stage();
    store_stage(0);
    advance();
    __syncthreads();
    int cur = 0, cnt = 0, ct = 0;  // stages of tile ct consumed
    for (int g = 0; g < total; ++g) {  // workgroup-uniform
        const bool more = g + 1 < total;
        if (more) load_stage();
        const float* xl = smem + cur * BUF;
        const float* al = xl + SW_KC * SW_NT;
#pragma unroll
        for (int kp = 0; kp < SW_KC / 2; ++kp) {
            const int kk = 2 * kp + half;
            float av[TA], bv[2];
#pragma unroll
            for (int t = 0; t < TA; ++t) av[t] = al[kk * LDA + t * 32 + j];
#pragma unroll
            for (int u = 0; u < 2; ++u) bv[u] = xl[kk * SW_NT + (wave * 2 + u) * 32 + j];
#pragma unroll
            for (int t = 0; t < TA; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[u], acc[t][u], 0, 0, 0);
        }
        if (++cnt == nblk) {  // the tile's products are complete (workgroup-uniform)
            const int nb = (t0 + ct) * SW_NT + wave * 64 + j;
            const bool ok[2] = {nb < N, nb + 32 < N};
            int stride = N;  // (opaque to the compiler: 16 TA row offsets hoisted out of the K loop would cost two registers each)
            asm volatile("" : "+s"(stride));
#pragma unroll
            for (int t = 0; t < TA; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (row < M && ok[u]) {
                            const int64_t at = (int64_t)row * stride + nb + 32 * u;
                            if constexpr (MODE <= 1) out[at] = acc[t][u][r];
                            else if constexpr (MODE == 2) out[at] = scale * acc[t][u][r];
                            else out[at] = out[at] + scale * acc[t][u][r];
                        }
                }
                if constexpr (RANGE) {
                    float mn[16], mx[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {  // a padded pixel holds a 0 that is no value of P
                        mn[r] = fminf(ok[0] ? acc[t][0][r] : INFINITY, ok[1] ? acc[t][1][r] : INFINITY);
                        mx[r] = fmaxf(ok[0] ? acc[t][0][r] : -INFINITY, ok[1] ? acc[t][1][r] : -INFINITY);
                    }
                    sw_fold<8>(mn, mx, lane & 1, 1);
                    sw_fold<4>(mn, mx, lane & 2, 2);
                    sw_fold<2>(mn, mx, lane & 4, 4);
                    sw_fold<1>(mn, mx, lane & 8, 8);
                    mn[0] = fminf(mn[0], __shfl_xor(mn[0], 16, 64));
                    mx[0] = fmaxf(mx[0], __shfl_xor(mx[0], 16, 64));
                    // the accumulator row this lane is left with: bit s of the lane chose the upper half of step s
                    const int r = ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
                    if ((lane & 16) == 0) {
                        const int lr = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        red[wave * MT + lr] = mn[0];
                        red[(4 + wave) * MT + lr] = mx[0];
                    }
                }
            }
            if constexpr (RANGE) {
                __syncthreads();
                if (tid < MT) {
                    const float lo = fminf(fminf(red[tid], red[MT + tid]), fminf(red[2 * MT + tid], red[3 * MT + tid]));
                    const float hi = fmaxf(fmaxf(red[4 * MT + tid], red[5 * MT + tid]), fmaxf(red[6 * MT + tid], red[7 * MT + tid]));
                    run[tid] = ct == 0 ? lo : fminf(run[tid], lo);
                    run[MT + tid] = ct == 0 ? hi : fmaxf(run[MT + tid], hi);
                }
            }
            clear();
            cnt = 0;
            ++ct;
        }
        if (more) {
            store_stage(cur ^ 1);
            advance();
        }
        __syncthreads();
        cur ^= 1;
    }
    if constexpr (RANGE) {
        if (tid < MT && m0 + tid < M) {  // run[] was last written by this thread
            float* mm = minmax + ((int64_t)(m0 + tid) * gridDim.x + blockIdx.x) * 2;
            mm[0] = run[tid];
            mm[1] = run[MT + tid];
        }
    }
}

template <int TA, bool RANGE>
static __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, TA == 4 ? 2 : 3)))  // TA = 4: 256 registers a lane
swd_project_kernel(const float* __restrict__ dirs, const float* __restrict__ f, float* __restrict__ proj, int D, int C, int N, int span, int ntiles,
                   float* __restrict__ minmax, int* __restrict__ state, int bins) {
    sw_product<TA, RANGE ? 1 : 0>(dirs, f, proj, D, C, N, span, ntiles, minmax, state, bins, 1.f);
}

template <int TA, bool ACC>
static __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, TA == 4 ? 2 : 3)))
swd_back_kernel(const float* __restrict__ dirs_t, const float* __restrict__ g, float* __restrict__ gx, int C, int D, int N, int span, int ntiles,
                const float* __restrict__ upstream, double coef) {
    const float scale = (float)(coef * (upstream ? (double)upstream[0] : 1.0));
    sw_product<TA, ACC ? 3 : 2>(dirs_t, g, gx, C, D, N, span, ntiles, nullptr, nullptr, 0, scale);
}

// fh_sweep over a chunk that the operations also write: every element is read once, by the thread that then writes it
template <class Op1, class Op4>
__device__ __forceinline__ void sw_sweep(float* p, int n, Op1&& op1, Op4&& op4) {
    const int tid = threadIdx.x;
    const int head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2));
    const int nq = (n - head) >> 2;
    const int tail = head + 4 * nq;
    for (int i = tid; i < head; i += FH_THREADS) op1(i, p[i]);
    const fh_f32x4* q4 = reinterpret_cast<const fh_f32x4*>(p + head);
    for (int q0 = tid; q0 < nq; q0 += FH_UNROLL * FH_THREADS) {
        fh_f32x4 v[FH_UNROLL];
#pragma unroll
        for (int u = 0; u < FH_UNROLL; ++u)
            if (q0 + u * FH_THREADS < nq) v[u] = q4[q0 + u * FH_THREADS];
#pragma unroll
        for (int u = 0; u < FH_UNROLL; ++u)
            if (q0 + u * FH_THREADS < nq) op4(head + 4 * (q0 + u * FH_THREADS), v[u]);
    }
    if (tid < n - tail) op1(tail + tid, p[tail + tid]);  // fewer than four
}

static __global__ void __launch_bounds__(FH_THREADS)
swd_resid_kernel(float* p, const float* __restrict__ table, const int* __restrict__ state, double* __restrict__ partial, int N, int chunks,
                 int chunk, int bins, int knots) {
    __shared__ float tab[FH_KNOTS_MAX];
    __shared__ int cum[FH_BINS_MAX + 1];
    __shared__ double scratch[16];
    const int c = blockIdx.x / chunks, ks = blockIdx.x - c * chunks;
    const int p0 = ks * chunk;
    const int n = min(chunk, N - p0);
    float lo, inv;
    fh_stage(table, state, c, bins, knots, tab, cum, &lo, &inv);
    const float nf = (float)N;
    float* row = p + (int64_t)c * N + p0;
    double acc = 0.0;
    auto resid = [&](float v) {
        const float d = v - fh_match(v, lo, inv, bins, knots, nf, cum, tab);
        acc += (double)d * (double)d;
        return d;
    };
    auto op1 = [&](int i, float v) { row[i] = resid(v); };
    auto op4 = [&](int i, fh_f32x4 v) {
        fh_f32x4 g;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = resid(v[k]);
        *reinterpret_cast<fh_f32x4*>(row + i) = g;
    };
    sw_sweep(row, n, op1, op4);
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[(int64_t)c * chunks + ks] = acc;
}

static bool sw_bins_ok(int bins) { return bins >= FH_BINS_MIN && bins <= FH_BINS_MAX; }

// bytes of the partial sums (first) and of the slabs (behind them) for D directions over n pixels
static void sw_workspace(int d, int64_t n, size_t* partial_bytes, size_t* slab_bytes) {
    int chunks, chunk, ntiles, span, slabs;
    fh_plan(d, n, &chunks, &chunk);
    sw_plan(d, n, &ntiles, &span, &slabs);
    *partial_bytes = (size_t)d * chunks * sizeof(double);
    *slab_bytes = (size_t)d * slabs * 2 * sizeof(float);
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_swd_supported(int c, int d, int h, int w, int bins, int knots) {
    return sw_shape_ok(c, d, h, w) && fh_shape_ok(d, h, w, bins, knots) ? 1 : 0;
}

size_t maua_swd_workspace_bytes(int c, int d, int h, int w, int bins, int knots) {
    if (!maua_swd_supported(c, d, h, w, bins, knots)) return 0;
    size_t partial, slab;
    sw_workspace(d, (int64_t)h * w, &partial, &slab);
    return partial + slab;
}

size_t maua_swd_state_bytes(int d, int bins) {
    if (d < 1 || d > SW_CMAX || !sw_bins_ok(bins)) return 0;
    return (size_t)d * (bins + 3) * 4;
}

int maua_swd_project(const float* f, const float* dirs, float* proj, void* state, int c, int d, int h, int w, int bins, void* workspace,
                     size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(f && dirs && proj && (!state || workspace), MAUA_E_INVAL, "swd_project: null pointer");
    MAUA_REQUIRE(sw_shape_ok(c, d, h, w) && (!state || sw_bins_ok(bins)), MAUA_E_UNSUPPORTED,
                 "swd_project: %d channels and %d directions (1 .. %d), %d x %d pixels (below 2^30), %d bins (%d .. %d)", c, d, SW_CMAX, h, w, bins,
                 FH_BINS_MIN, FH_BINS_MAX);
    const int N = h * w;
    int ntiles, span, slabs;
    sw_plan(d, N, &ntiles, &span, &slabs);
    float* minmax = nullptr;
    if (state) {
        size_t partial, slab;
        sw_workspace(d, N, &partial, &slab);
        MAUA_REQUIRE(workspace_bytes >= partial + slab, MAUA_E_WORKSPACE, "swd_project: workspace %zu < %zu", workspace_bytes, partial + slab);
        MAUA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL,
                     "swd_project: workspace (8 bytes) or state (4 bytes) misaligned");
        minmax = (float*)((char*)workspace + partial);
    }
    const int ta = sw_ta(d, N);
    const dim3 grid((unsigned)slabs, (unsigned)((d + 32 * ta - 1) / (32 * ta))), block(256);
    hipStream_t s = (hipStream_t)stream;
    int* st = (int*)state;
#define SW_PROJECT(TA, RANGE) hipLaunchKernelGGL((swd_project_kernel<TA, RANGE>), grid, block, 0, s, dirs, f, proj, d, c, N, span, ntiles, minmax, st, bins)
    if (state) {
        if (ta == 1) SW_PROJECT(1, true);
        else if (ta == 2) SW_PROJECT(2, true);
        else SW_PROJECT(4, true);
    } else {
        if (ta == 1) SW_PROJECT(1, false);
        else if (ta == 2) SW_PROJECT(2, false);
        else SW_PROJECT(4, false);
    }
#undef SW_PROJECT
    return check_launch("swd_project_kernel");
}

int maua_swd_match(float* proj_inout, const float* table, void* state, float* loss, int d, int h, int w, int bins, int knots, void* workspace,
                   size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(proj_inout && table && state && loss && workspace, MAUA_E_INVAL, "swd_match: null pointer");
    MAUA_REQUIRE(sw_shape_ok(1, d, h, w) && fh_shape_ok(d, h, w, bins, knots), MAUA_E_UNSUPPORTED,
                 "swd_match: %d directions (1 .. %d), %d x %d pixels (below 2^30), %d bins (%d .. %d), %d knots (%d .. %d)", d, SW_CMAX, h, w, bins,
                 FH_BINS_MIN, FH_BINS_MAX, knots, FH_KNOTS_MIN, FH_KNOTS_MAX);
    const int N = h * w;
    size_t pbytes, slab;
    sw_workspace(d, N, &pbytes, &slab);
    MAUA_REQUIRE(workspace_bytes >= pbytes + slab, MAUA_E_WORKSPACE, "swd_match: workspace %zu < %zu", workspace_bytes, pbytes + slab);
    MAUA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL,
                 "swd_match: workspace (8 bytes) or state (4 bytes) misaligned");
    int chunks, chunk, ntiles, span, slabs;
    fh_plan(d, N, &chunks, &chunk);
    sw_plan(d, N, &ntiles, &span, &slabs);
    double* partial = (double*)workspace;
    const float* minmax = (const float*)((char*)workspace + pbytes);
    int* st = (int*)state;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)d * (unsigned)chunks), block(FH_THREADS);  // at most 4096 + 2048
    hipLaunchKernelGGL(fh_count_kernel, grid, block, 0, s, (const float*)proj_inout, st, minmax, N, chunks, chunk, bins, slabs);
    int rc = check_launch("fh_count_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_scan_kernel, dim3(d), block, 0, s, st, minmax, slabs, bins);
    rc = check_launch("fh_scan_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(swd_resid_kernel, grid, block, 0, s, proj_inout, table, (const int*)st, partial, N, chunks, chunk, bins, knots);
    rc = check_launch("swd_resid_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_finish_kernel, dim3(1), block, 0, s, (const double*)partial, d * chunks, 1.0 / ((double)d * (double)N), loss);
    return check_launch("fh_finish_kernel");
}

int maua_swd_bwd(const float* g, const float* dirs_t, const float* upstream, double coef, float* gx, int c, int d, int h, int w, int accumulate,
                 maua_stream_t stream) {
    MAUA_REQUIRE(g && dirs_t && gx, MAUA_E_INVAL, "swd_bwd: null pointer");
    MAUA_REQUIRE(sw_shape_ok(c, d, h, w), MAUA_E_UNSUPPORTED, "swd_bwd: %d channels and %d directions (1 .. %d), %d x %d pixels (below 2^30)", c, d,
                 SW_CMAX, h, w);
    const int N = h * w;
    int ntiles, span, slabs;
    sw_plan(c, N, &ntiles, &span, &slabs);
    const int ta = sw_ta(c, N);
    const dim3 grid((unsigned)slabs, (unsigned)((c + 32 * ta - 1) / (32 * ta))), block(256);
    hipStream_t s = (hipStream_t)stream;
#define SW_BACK(TA, ACC) hipLaunchKernelGGL((swd_back_kernel<TA, ACC>), grid, block, 0, s, dirs_t, g, gx, c, d, N, span, ntiles, upstream, coef)
    if (accumulate) {
        if (ta == 1) SW_BACK(1, true);
        else if (ta == 2) SW_BACK(2, true);
        else SW_BACK(4, true);
    } else {
        if (ta == 1) SW_BACK(1, false);
        else if (ta == 2) SW_BACK(2, false);
        else SW_BACK(4, false);
    }
#undef SW_BACK
    return check_launch("swd_back_kernel");
}

}  // extern "C"
