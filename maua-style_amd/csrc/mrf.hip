// MRF patch-matching style loss (Li & Wand 2016, "Combining Markov Random Fields and Convolutional Neural Networks for Image Synthesis"):
// every 3x3 patch of a style layer's activation is pulled towards its nearest style patch under normalised cross-correlation (DESIGN.md
// section 16).  One frame F[C][H][W], H, W >= 3:
//     query grid   Hq = H - 2, Wq = W - 2, Q = Hq Wq, q = yq Wq + xq;   Psi_q(F)[c][dy][dx] = F[c][yq + dy][xq + dx], dy, dx in 0 .. 2
//     style bank   a map S[C][Hs][Ws], origin[P] (int32, = ys Ws + xs, the whole patch inside the map) and
//                  inv[P] (fp32) = 1 / ||Psi_p(S)||, the squared norm summed in fp64 and rounded once; patches of norm 0 are never listed
//     score(q, p) = inv[p] sum_{c,dy,dx} F[c][yq+dy][xq+dx] S[c][origin[p] + dy Ws + dx]
//     nn[q]       = the p of the largest score; among bit-equal scores the lowest p       (the query's own norm does not change the arg-max)
//     loss        = 1 / (9 C Q) sum_q sum_{c,dy,dx} (F[c][yq+dy][xq+dx] - S[c][origin[nn[q]] + dy Ws + dx])^2
//     gx[c][y][x] (+)= coef upstream sum over (dy, dx) with 0 <= y - dy < Hq, 0 <= x - dx < Wq of
//                      (F[c][y][x] - S[c][origin[nn[(y-dy) Wq + (x-dx)]] + dy Ws + dx])                            (nn is a constant)
// Launch plan.
//   bank      mrf_bank_kernel    one wave per style patch: the 9 C squares in fp64, a shuffle tree of fixed shape, inv[p] rounded once
//   forward   mrf_match_kernel   implicit GEMM with K = 9 C on the fp32 matrix cores (v_mfma_f32_32x32x2f32).  A workgroup owns 256 queries
//                                (a wave 64 of them) and one slice of the bank, which it walks in tiles of 128 style patches; a stage is one
//                                (tap, block of 16 channels): 16 x 256 values of F and 16 x 128 of S through double-buffered LDS (48 KB, two
//                                workgroups per CU by registers), read back as in gs_bwd_kernel - row k, consecutive lanes consecutive
//                                columns, no bank conflict.  A wave holds 128 patches x 64 queries in 4 x 2 accumulators; a lane owns two
//                                queries and, after every style tile, folds its 64 scores (times inv) into a running (score, p) per query:
//                                strictly greater wins, or equal with a lower p.  The Q x P scores are never written.  The two lanes of a
//                                query are folded with one shuffle at the end and the slice's winners go to the workspace.  F is staged
//                                again for every style tile, 43 floating-point operations per staged byte: with tiles of 64 patches (26
//                                per byte) the staging traffic, not the matrix cores, set the time (profiles/bench_mrf.md).
//             mrf_merge_kernel   a thread per query takes the slices' winners in slice order (ascending p) and writes `state`
//             mrf_loss_kernel    a thread per element of a block of channels of one pixel: reads F once, gathers the up to 9 style values
//                                of the query patches that cover the pixel; the workgroup's sum in fp64 to the workspace
//             mrf_finish_kernel  one workgroup adds the partial sums in a fixed order (fp64) and writes loss[0]
//   backward  mrf_bwd_kernel     the same gather, one launch: reads F once, writes gx once (read-modify-write when accumulating)
// The slices of the bank are a function of (Q, P) alone (mrf_plan), the merge takes them in order, no launch uses a float atomic: the same
// inputs give the same bits.  A padded query, a padded patch or a channel past C is decided from indices before any address is formed; it
// contributes zeros to the products and is never compared, so it cannot win.
// No packed fp32 instructions beside the MFMAs (build_native._file_flags).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <limits.h>
#include <stdlib.h>

#include "fp16x3.hpp"

namespace maua {

constexpr int MRF_KC = 16;    // channels per stage
constexpr int MRF_QT = 256;   // queries per workgroup
constexpr int MRF_PT = 128;   // style patches per tile
constexpr int MRF_TA = MRF_PT / 32;             // 32-patch blocks of a tile: a wave holds MRF_TA x 2 accumulators
constexpr int MRF_SW = MRF_KC * MRF_PT / 256;   // values of S a thread stages
constexpr int MRF_BUF = MRF_KC * MRF_QT + MRF_KC * MRF_PT;  // floats of one LDS buffer
constexpr int MRF_SMAX = 64;  // most slices of the bank
constexpr int MRF_WGS = 4096; // workgroups the match aims at: 8 rounds of two per CU
constexpr int MRF_GWGS = 2048;  // workgroups the gather launches aim at
constexpr int MRF_CMAX = 1024, MRF_PMAX = 1 << 20;

static bool mrf_shape_ok(int c, int h, int w, int hs, int ws, int p) {
    return c >= 1 && c <= MRF_CMAX && h >= 3 && w >= 3 && hs >= 3 && ws >= 3 && (int64_t)h * w < (1ll << 30) && (int64_t)hs * ws < (1ll << 30) &&
           p >= 1 && p <= MRF_PMAX;
}

// slices of the bank and their length in tiles of MRF_PT patches: about MRF_WGS workgroups, at most MRF_SMAX slices - a function of (Q, P)
static void mrf_plan(int64_t q, int p, int* slices, int* tiles_per_slice) {
    const int64_t qtiles = (q + MRF_QT - 1) / MRF_QT;
    const int tiles = (p + MRF_PT - 1) / MRF_PT;
    int64_t want = (MRF_WGS + qtiles - 1) / qtiles;
    if (want > MRF_SMAX) want = MRF_SMAX;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const int per = (int)((tiles + want - 1) / want);
    *tiles_per_slice = per;
    *slices = (tiles + per - 1) / per;
}

// channel blocks of the gather launches: about MRF_GWGS workgroups of 256 pixels x `cper` channels - a function of (C, H W)
static void mrf_gather_plan(int c, int64_t hw, int* pblocks, int* cchunks, int* cper) {
    const int64_t pb = (hw + 255) / 256;
    int64_t want = (MRF_GWGS + pb - 1) / pb;
    if (want > c) want = c;
    if (want < 1) want = 1;
    const int per = (int)((c + want - 1) / want);
    *pblocks = (int)pb;
    *cper = per;
    *cchunks = (c + per - 1) / per;
}

__device__ __forceinline__ bool mrf_better(float s, int p, float bs, int bp) { return s > bs || (s == bs && p < bp); }

// grid ceil(P / 4): wave w of a workgroup owns patch 4 blockIdx.x + w
__global__ void __launch_bounds__(256)
mrf_bank_kernel(const float* __restrict__ s, const int* __restrict__ origin, float* __restrict__ inv, int C, int HsWs, int Ws, int P) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;  // (wave-uniform)
    const int o = origin[p];
    double acc = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float* sc = s + (int64_t)c * HsWs + o;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const double v = (double)sc[dy * Ws + dx];
                acc += v * v;
            }
    }
    acc = wave_sum(acc);
    if (lane == 0) inv[p] = acc > 0.0 ? (float)(1.0 / sqrt(acc)) : 0.f;
}

// grid (query tiles, slices).  wscore / wp: [slice][Q] - the slice's winner of every query.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))  // two workgroups per CU: 256 registers a lane
mrf_match_kernel(const float* __restrict__ f, const float* __restrict__ s, const int* __restrict__ origin, const float* __restrict__ inv,
                 float* __restrict__ wscore, int* __restrict__ wp, int C, int H, int W, int HsWs, int Ws, int P, int Q, int Wq,
                 int tiles_per_slice) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[MRF_KC][256] + Wl[MRF_KC][MRF_PT])
    float* smem = smem_f32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int64_t HW = (int64_t)H * W;
    const int slice = blockIdx.y;
    const int pbeg = slice * tiles_per_slice * MRF_PT;  // < P (mrf_plan)
    const int pend = min(P, pbeg + tiles_per_slice * MRF_PT);
    const int ntile = (pend - pbeg + MRF_PT - 1) / MRF_PT;
    const int nblk = (C + MRF_KC - 1) / MRF_KC;
    const int spt = 9 * nblk;  // stages per style tile
    const int total = ntile * spt;

    // this thread's query of every F stage, and its patch of every S stage
    const int qload = blockIdx.x * MRF_QT + tid;
    const bool qok = qload < Q;
    const int qbase = qok ? (qload / Wq) * W + (qload % Wq) : 0;
    const int pl = tid & (MRF_PT - 1), prow = tid / MRF_PT;
    int lt = 0, tap = 0, cb = 0;  // the stage to load next
    int porg = -1;                // origin of this thread's patch in tile lt, -1: padded
    auto fetch_origin = [&]() {
        const int p = pbeg + lt * MRF_PT + pl;
        porg = (lt < ntile && p < pend) ? origin[p] : -1;
    };
    fetch_origin();

    float rx[MRF_KC], rw[MRF_SW];
    auto load_stage = [&]() {
        const int dy = tap / 3, dx = tap - 3 * dy;
        const int k0 = cb * MRF_KC;
        const float* fq = f + qbase + dy * W + dx;
#pragma unroll
        for (int i = 0; i < MRF_KC; ++i) {
            const int c = k0 + i;
            rx[i] = (qok && c < C) ? fq[(int64_t)c * HW] : 0.f;
        }
        const int so = porg + dy * Ws + dx;
#pragma unroll
        for (int i = 0; i < MRF_SW; ++i) {
            const int c = k0 + prow + (256 / MRF_PT) * i;
            rw[i] = (porg >= 0 && c < C) ? s[(int64_t)c * HsWs + so] : 0.f;
        }
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * MRF_BUF;
        float* wl = xl + MRF_KC * MRF_QT;
#pragma unroll
        for (int i = 0; i < MRF_KC; ++i) xl[i * MRF_QT + tid] = rx[i];
#pragma unroll
        for (int i = 0; i < MRF_SW; ++i) wl[(prow + (256 / MRF_PT) * i) * MRF_PT + pl] = rw[i];
    };
    auto advance = [&]() {
        if (++cb == nblk) {
            cb = 0;
            if (++tap == 9) {
                tap = 0;
                ++lt;
                fetch_origin();
            }
        }
    };

    f32x16 acc[MRF_TA][2];
    auto clear = [&]() {
#pragma unroll
        for (int t = 0; t < MRF_TA; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;
    };
    clear();
    float bs[2] = {-INFINITY, -INFINITY};
    int bp[2] = {INT_MAX, INT_MAX};

    load_stage();
    store_stage(0);
    advance();
    __syncthreads();
    int cur = 0, cnt = 0, ct = 0;  // stages of style tile ct consumed
    for (int g = 0; g < total; ++g) {  // workgroup-uniform
        const bool more = g + 1 < total;
        if (more) load_stage();
        const float* xl = smem + cur * MRF_BUF;
        const float* wl = xl + MRF_KC * MRF_QT;
#pragma unroll
        for (int kp = 0; kp < MRF_KC / 2; ++kp) {
            const int kk = 2 * kp + half;
            float a[MRF_TA], b[2];
#pragma unroll
            for (int t = 0; t < MRF_TA; ++t) a[t] = wl[kk * MRF_PT + t * 32 + j];
#pragma unroll
            for (int u = 0; u < 2; ++u) b[u] = xl[kk * MRF_QT + (wave * 2 + u) * 32 + j];
#pragma unroll
            for (int t = 0; t < MRF_TA; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
        if (++cnt == spt) {  // the tile's scores are complete: fold them into the running winners, rows in ascending p
            const int p0 = pbeg + ct * MRF_PT;
#pragma unroll
            for (int t = 0; t < MRF_TA; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = p0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (p < pend) {  // a padded patch is never compared
                        const float ip = inv[p];
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const float sc = acc[t][u][r] * ip;
                            if (mrf_better(sc, p, bs[u], bp[u])) {
                                bs[u] = sc;
                                bp[u] = p;
                            }
                        }
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
#pragma unroll
    for (int u = 0; u < 2; ++u) {  // the other half of the query's rows sits 32 lanes away
        const float os = __shfl_xor(bs[u], 32, 64);
        const int op = __shfl_xor(bp[u], 32, 64);
        if (mrf_better(os, op, bs[u], bp[u])) {
            bs[u] = os;
            bp[u] = op;
        }
        const int q = blockIdx.x * MRF_QT + (wave * 2 + u) * 32 + j;
        if (half == 0 && q < Q) {
            wscore[(int64_t)slice * Q + q] = bs[u];
            wp[(int64_t)slice * Q + q] = bp[u];
        }
    }
}

// a thread per query: the slices in order (their patches ascend), a later one wins only with a strictly greater score
__global__ void __launch_bounds__(256)
mrf_merge_kernel(const float* __restrict__ wscore, const int* __restrict__ wp, int* __restrict__ nn, float* __restrict__ best, int Q, int P,
                 int slices) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    float bs = wscore[q];
    int bp = wp[q];
    for (int sl = 1; sl < slices; ++sl) {
        const float sc = wscore[(int64_t)sl * Q + q];
        const int p = wp[(int64_t)sl * Q + q];
        if (mrf_better(sc, p, bs, bp)) {
            bs = sc;
            bp = p;
        }
    }
    if (bp < 0 || bp >= P) bp = 0;  // (every score a NaN: still an address inside the bank)
    nn[q] = bp;
    best[q] = bs;
}

// The query patches that cover pixel (y, x): bit k = 3 dy + dx of the mask is set where (y - dy, x - dx) is a query, and off[k] is then the
// offset inside a channel of S of the style value that its nearest patch puts on the pixel.  Indices decide before any address is formed.
struct MrfTaps {
    unsigned mask;
    int off[9];
};
__device__ __forceinline__ MrfTaps mrf_taps(const int* __restrict__ nn, const int* __restrict__ origin, int y, int x, int Hq, int Wq, int Ws,
                                            int P) {
    MrfTaps t;
    t.mask = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int k = 3 * dy + dx, yq = y - dy, xq = x - dx;
            t.off[k] = 0;
            if (yq >= 0 && yq < Hq && xq >= 0 && xq < Wq) {
                const int p = min(max(nn[yq * Wq + xq], 0), P - 1);
                t.off[k] = origin[p] + dy * Ws + dx;
                t.mask |= 1u << k;
            }
        }
    return t;
}

// grid (pixel blocks, channel chunks); partial[blockIdx.y gridDim.x + blockIdx.x]
__global__ void __launch_bounds__(256)
mrf_loss_kernel(const float* __restrict__ f, const float* __restrict__ s, const int* __restrict__ origin, const int* __restrict__ nn,
                double* __restrict__ partial, int C, int H, int W, int HsWs, int Ws, int P, int cper) {
    __shared__ double scratch[16];
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (pix < HW) {
        const int y = pix / W, x = pix - y * W;
        const MrfTaps t = mrf_taps(nn, origin, y, x, H - 2, W - 2, Ws, P);
        const int c0 = blockIdx.y * cper, c1 = min(C, c0 + cper);
        for (int c = c0; c < c1; ++c) {
            const float v = f[(int64_t)c * HW + pix];
            const float* sc = s + (int64_t)c * HsWs;
            float sq = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if ((t.mask >> k) & 1u) {
                    const float d = v - sc[t.off[k]];
                    sq += d * d;
                }
            acc += (double)sq;
        }
    }
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// one workgroup: thread t adds the partial sums t, t + 256, ... in order, then a tree of fixed shape
__global__ void __launch_bounds__(256)
mrf_finish_kernel(const double* __restrict__ partial, int n, double scale, float* __restrict__ loss) {
    __shared__ double scratch[16];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += partial[i];
    v = block_sum(v, scratch);
    if (threadIdx.x == 0) loss[0] = (float)(v * scale);
}

template <bool ACC>
__global__ void __launch_bounds__(256)
mrf_bwd_kernel(const float* __restrict__ f, const float* __restrict__ s, const int* __restrict__ origin, const int* __restrict__ nn,
               const float* __restrict__ upstream, double coef, float* __restrict__ gx, int C, int H, int W, int HsWs, int Ws, int P, int cper) {
    const int HW = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= HW) return;
    const float scale = (float)(coef * (upstream ? (double)upstream[0] : 1.0));
    const int y = pix / W, x = pix - y * W;
    const MrfTaps t = mrf_taps(nn, origin, y, x, H - 2, W - 2, Ws, P);
    const int c0 = blockIdx.y * cper, c1 = min(C, c0 + cper);
    for (int c = c0; c < c1; ++c) {
        const int64_t at = (int64_t)c * HW + pix;
        const float v = f[at];
        const float* sc = s + (int64_t)c * HsWs;
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if ((t.mask >> k) & 1u) sum += v - sc[t.off[k]];
        const float g = scale * sum;
        gx[at] = ACC ? gx[at] + g : g;
    }
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_mrf_supported(int c, int h, int w, int hs, int ws, int p) { return mrf_shape_ok(c, h, w, hs, ws, p) ? 1 : 0; }

size_t maua_mrf_workspace_bytes(int c, int h, int w, int hs, int ws, int p) {
    if (!mrf_shape_ok(c, h, w, hs, ws, p)) return 0;
    const int64_t q = (int64_t)(h - 2) * (w - 2);
    int slices, per, pblocks, cchunks, cper;
    mrf_plan(q, p, &slices, &per);
    mrf_gather_plan(c, (int64_t)h * w, &pblocks, &cchunks, &cper);
    // partial sums of the loss, then the slices' winners: scores and patches
    return (size_t)pblocks * cchunks * sizeof(double) + (size_t)slices * q * (sizeof(float) + sizeof(int));
}

size_t maua_mrf_state_bytes(int h, int w) {
    if (h < 3 || w < 3 || (int64_t)h * w >= (1ll << 30)) return 0;
    return (size_t)(h - 2) * (w - 2) * (sizeof(int) + sizeof(float));  // nn[Q], best[Q]
}

int maua_mrf_bank(const float* s, const int* origin, float* inv, int c, int hs, int ws, int p, maua_stream_t stream) {
    MAUA_REQUIRE(s && origin && inv, MAUA_E_INVAL, "mrf_bank: null pointer");
    MAUA_REQUIRE(mrf_shape_ok(c, 3, 3, hs, ws, p), MAUA_E_UNSUPPORTED, "mrf_bank: %d channels (1 .. %d), a %d x %d map (3 .. , below 2^30), %d patches (1 .. %d)",
                 c, MRF_CMAX, hs, ws, p, MRF_PMAX);
    hipLaunchKernelGGL(mrf_bank_kernel, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, origin, inv, c, hs * ws, ws, p);
    return check_launch("mrf_bank_kernel");
}

int maua_mrf_fwd(const float* f, const float* s, const int* origin, const float* inv, void* state, float* loss, int c, int h, int w, int hs, int ws,
                 int p, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(f && s && origin && inv && state && loss && workspace, MAUA_E_INVAL, "mrf_fwd: null pointer");
    MAUA_REQUIRE(mrf_shape_ok(c, h, w, hs, ws, p), MAUA_E_UNSUPPORTED,
                 "mrf_fwd: %d channels (1 .. %d), %d x %d pixels and a %d x %d style map (3 .. , below 2^30), %d patches (1 .. %d)", c, MRF_CMAX, h, w,
                 hs, ws, p, MRF_PMAX);
    const size_t need = maua_mrf_workspace_bytes(c, h, w, hs, ws, p);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "mrf_fwd: workspace %zu < %zu", workspace_bytes, need);
    MAUA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL,
                 "mrf_fwd: workspace (8 bytes) or state (4 bytes) misaligned");
    const int Hq = h - 2, Wq = w - 2, Q = Hq * Wq;
    int slices, per, pblocks, cchunks, cper;
    mrf_plan(Q, p, &slices, &per);
    mrf_gather_plan(c, (int64_t)h * w, &pblocks, &cchunks, &cper);
    double* partial = (double*)workspace;
    float* wscore = (float*)(partial + (size_t)pblocks * cchunks);
    int* wp = (int*)(wscore + (size_t)slices * Q);
    int* nn = (int*)state;
    float* best = (float*)(nn + Q);
    hipStream_t st = (hipStream_t)stream;
    constexpr int lds = 2 * MRF_BUF * (int)sizeof(float);
    static unsigned long long opted = 0;
    const hipError_t e = opt_in_dynamic_lds(reinterpret_cast<const void*>(mrf_match_kernel), lds, &opted);
    MAUA_REQUIRE(e == hipSuccess, (int)e, "mrf_fwd: %d bytes of LDS: %s", lds, hipGetErrorString(e));
    hipLaunchKernelGGL(mrf_match_kernel, dim3((unsigned)((Q + MRF_QT - 1) / MRF_QT), (unsigned)slices), dim3(256), lds, st, f, s, origin, inv, wscore,
                       wp, c, h, w, hs * ws, ws, p, Q, Wq, per);
    int rc = check_launch("mrf_match_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(mrf_merge_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, (const float*)wscore, (const int*)wp, nn, best, Q, p,
                       slices);
    rc = check_launch("mrf_merge_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(mrf_loss_kernel, dim3((unsigned)pblocks, (unsigned)cchunks), dim3(256), 0, st, f, s, origin, (const int*)nn, partial, c, h, w,
                       hs * ws, ws, p, cper);
    rc = check_launch("mrf_loss_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(mrf_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, pblocks * cchunks, 1.0 / (9.0 * (double)c * (double)Q),
                       loss);
    return check_launch("mrf_finish_kernel");
}

int maua_mrf_bwd(const float* f, const float* s, const int* origin, const void* state, const float* upstream, double coef, float* gx, int c, int h,
                 int w, int hs, int ws, int p, int accumulate, maua_stream_t stream) {
    MAUA_REQUIRE(f && s && origin && state && gx, MAUA_E_INVAL, "mrf_bwd: null pointer");
    MAUA_REQUIRE(mrf_shape_ok(c, h, w, hs, ws, p), MAUA_E_UNSUPPORTED,
                 "mrf_bwd: %d channels (1 .. %d), %d x %d pixels and a %d x %d style map (3 .. , below 2^30), %d patches (1 .. %d)", c, MRF_CMAX, h, w,
                 hs, ws, p, MRF_PMAX);
    MAUA_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL, "mrf_bwd: state misaligned");
    int pblocks, cchunks, cper;
    mrf_gather_plan(c, (int64_t)h * w, &pblocks, &cchunks, &cper);
    const dim3 grid((unsigned)pblocks, (unsigned)cchunks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (accumulate)
        hipLaunchKernelGGL(mrf_bwd_kernel<true>, grid, block, 0, st, f, s, origin, (const int*)state, upstream, coef, gx, c, h, w, hs * ws, ws, p, cper);
    else
        hipLaunchKernelGGL(mrf_bwd_kernel<false>, grid, block, 0, st, f, s, origin, (const int*)state, upstream, coef, gx, c, h, w, hs * ws, ws, p, cper);
    return check_launch("mrf_bwd_kernel");
}

}  // extern "C"
