// Shifted Gram matrices (Berger & Memisevic 2016, "Incorporating long-range consistency in CNN-based texture generation"): for S
// translations (axis_s, delta_s) of one style layer with activation F[C][H W], X = F - mu (mu: the map's row means in the covariance form,
// else 0) and flat pixel index p = y W + x
//     G_s[c][k] = scale_s sum_{p valid for s} X[c][p + off_s] X[k][p]
// off_s = delta_s, valid: x < W - delta_s (axis 0);  off_s = delta_s W, valid: p < (H - delta_s) W (axis 1).  G_s is NOT symmetric.
// Backward, D_s = dL/dG_s as given (not symmetrised):
//     gx[c][q] (+)= sum_s coef_s ( [q - off_s valid] sum_k D_s[c][k] X[k][q - off_s] + [q valid] sum_k D_s[k][c] X[k][q + off_s] ).
//
// Forward: gram_guided.hip's fp32-MFMA split-K kernel with the shift as the third grid dimension and ALL tile pairs.  A stage writes two
// operands to LDS, X at p + off_s and X at p, with zeros where the pair is invalid; the finishing kernel adds the slabs in index order
// (fp64) and applies scale_s: deterministic, no float atomics.  The split of the pixel range depends on (C, H W) only, so a shift has the
// same bits alone or among others.
// Backward: gg_bwd_kernel's layout (64 output channels x 256 pixels per workgroup, 32 input channels per double-buffered LDS stage); every
// shift gives two runs of stages of one accumulation, D_s^T against X read at q - off_s and D_s against X read at q + off_s.  D_s^T is D_s
// written to LDS transposed, never to memory.
// No load leaves F: the validity mask of a pixel quad is computed from indices first and decides which addresses are formed at all.
// For the fused engine: a finishing kernel that also forms D_s = grad_scale_s (G_s - T_s) and the shifts' loss as one ledger record
// (gs_finish_mse_kernel), and a ReLU mask in the backward kernel's epilogue (gs_bwd_kernel's MASK flag).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <stdlib.h>

#include "fp16x3.hpp"

namespace maua {

constexpr int GS_T = 64;         // tile edge (channels)
constexpr int GS_K = 64;         // pixels per stage
constexpr int GS_RS = GS_K + 4;  // LDS row stride (floats), as gram_guided.hip
constexpr int GS_SMAX = 16;      // most shifts per call
constexpr int GS_KMAX = 256;     // most slabs per (shift, tile pair)

typedef float gs_f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct GsShifts {  // launch argument: the host arrays of one call
    int axis[GS_SMAX], delta[GS_SMAX];
    double factor[GS_SMAX];  // scale_s (forward) / coef_s (backward)
};

// bit k: pixel p + k lies in [lo, hi) and, with `cols`, its column in [clo, chi).  p >= 0 and below 2^30.
__device__ __forceinline__ unsigned gs_mask4(int64_t p, int64_t lo, int64_t hi, bool cols, int W, int clo, int chi) {
    unsigned m = 0;
    int col = cols ? (int)p % W : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool ok = p + k >= lo && p + k < hi;
        if (cols) {
            ok = ok && col >= clo && col < chi;
            if (++col == W) col = 0;
        }
        if (ok) m |= 1u << k;
    }
    return m;
}

// row[p + k] - mu for the elements k of the mask, 0 for the others; only the mask's addresses are formed
__device__ __forceinline__ f32x4 gs_load4(const float* __restrict__ row, int64_t p, unsigned m, float mu) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m == 15u) {
        v = *reinterpret_cast<const gs_f32x4u*>(row + p);
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
__device__ __forceinline__ f32x4 gs_load4_end(const float* __restrict__ row, int64_t p, int64_t end) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p + 4 <= end) {
        v = *reinterpret_cast<const gs_f32x4u*>(row + p);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p + k < end) v[k] = row[p + k];
    }
    return v;
}

// One workgroup = one shift x one 64x64 tile pair (ti: rows of G, the operand read at p + off; tj: columns, read at p) x one slice of the
// plane; the four waves own a 32x32 block each.  Slabs: partial[((s npairs + pair) ksplit + ks) 64 64].
__global__ void __launch_bounds__(256)
gs_partial_kernel(const float* __restrict__ f, const float* __restrict__ mean, float* __restrict__ partial, GsShifts sh, int C, int H, int W,
                  int npairs, int ksplit, int64_t chunk) {
    __shared__ __attribute__((aligned(16))) float At[GS_T * GS_RS];
    __shared__ __attribute__((aligned(16))) float Bt[GS_T * GS_RS];
    const int s = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i32 = lane & 31, half = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const int ntile = (C + GS_T - 1) / GS_T;
    const int ti = blockIdx.x / ntile, tj = blockIdx.x % ntile;
    const int ks = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int axis = sh.axis[s], delta = sh.delta[s];
    const int64_t off = axis == 0 ? (int64_t)delta : (int64_t)delta * W;
    const int64_t vend = axis == 0 ? HW : (int64_t)(H - delta) * W;  // pairs start below vend
    const int64_t p_begin = (int64_t)ks * chunk;
    const int64_t p_end = min(min(HW, p_begin + chunk), vend);

    constexpr int NL = GS_T * GS_K / 4 / 256;  // 4 quads per tile per thread: rows tid / 16 + 16 q, pixels 4 (tid % 16) .. + 3
    const int r0 = tid >> 4, c4 = (tid & 15) * 4;
    float ma[NL], mb[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int rowa = ti * GS_T + r0 + 16 * q, rowb = tj * GS_T + r0 + 16 * q;
        ma[q] = (mean && rowa < C) ? mean[rowa] : 0.f;
        mb[q] = (mean && rowb < C) ? mean[rowb] : 0.f;
    }
    f32x4 ra[NL], rb[NL];
    auto load_stage = [&](int64_t p0) {
        const int64_t pp = p0 + c4;
        const unsigned m = gs_mask4(pp, 0, p_end, axis == 0, W, 0, W - delta);  // the pair (p, p + off): decided before any address
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int rowa = ti * GS_T + r0 + 16 * q, rowb = tj * GS_T + r0 + 16 * q;
            ra[q] = gs_load4(f + (int64_t)min(rowa, C - 1) * HW, pp + off, rowa < C ? m : 0u, ma[q]);
            rb[q] = gs_load4(f + (int64_t)min(rowb, C - 1) * HW, pp, rowb < C ? m : 0u, mb[q]);
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            *reinterpret_cast<f32x4*>(At + (r0 + 16 * q) * GS_RS + c4) = ra[q];
            *reinterpret_cast<f32x4*>(Bt + (r0 + 16 * q) * GS_RS + c4) = rb[q];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    if (p_begin < p_end) {  // workgroup-uniform
        load_stage(p_begin);
        for (int64_t p0 = p_begin; p0 < p_end; p0 += GS_K) {
            __syncthreads();  // previous stage fully consumed
            store_stage();
            __syncthreads();
            if (p0 + GS_K < p_end) load_stage(p0 + GS_K);
            const float* at = At + (wi * 32 + i32) * GS_RS + 4 * half;
            const float* bt = Bt + (wj * 32 + i32) * GS_RS + 4 * half;
#pragma unroll
            for (int q = 0; q < GS_K / 8; ++q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(at + 8 * q);
                const f32x4 b = *reinterpret_cast<const f32x4*>(bt + 8 * q);
#pragma unroll
                for (int cp = 0; cp < 4; ++cp) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cp], b[cp], acc, 0, 0, 0);
            }
        }
    }
    float* out = partial + (((int64_t)s * npairs + blockIdx.x) * ksplit + ks) * (GS_T * GS_T);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        out[row * GS_T + wj * 32 + i32] = acc[r];
    }
}

// grid (tile pairs, 16, S): every thread owns one element of the 64x64 tile, adds its slab values in index order (fp64) and applies the
// shift's scale.
__global__ void __launch_bounds__(256)
gs_finish_kernel(const float* __restrict__ partial, float* __restrict__ gram, GsShifts sh, int C, int npairs, int ksplit) {
    const int s = blockIdx.z;
    const int ntile = (C + GS_T - 1) / GS_T;
    const int ti = blockIdx.x / ntile, tj = blockIdx.x % ntile;
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int er = e / GS_T, ec = e % GS_T;
    const float* base = partial + ((int64_t)s * npairs + blockIdx.x) * ksplit * (GS_T * GS_T) + e;
    double sd = 0.0;
    int k = 0;
    for (; k + 7 < ksplit; k += 8) {  // eight loads in flight, the additions in the order of a plain loop
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[(int64_t)(k + u) * (GS_T * GS_T)];
#pragma unroll
        for (int u = 0; u < 8; ++u) sd += (double)v[u];
    }
    for (; k < ksplit; ++k) sd += (double)base[(int64_t)k * (GS_T * GS_T)];
    const int gi = ti * GS_T + er, gj = tj * GS_T + ec;
    if (gi < C && gj < C) gram[((int64_t)s * C + gi) * C + gj] = (float)(sd * sh.factor[s]);
}

// gs_finish_kernel and the MSE against the shifts' targets in one launch: grid (tile pairs, 16 / FQ, S), every thread owns FQ elements of the
// 64x64 tile (e = 256 (FQ blockIdx.y + u) + tid).  Each element's slab values are added in index order in fp64 exactly as gs_finish_kernel
// adds them (the same bits); the target elements are requested first, so they arrive beside the slabs and not behind them, and the loads
// of the thread's FQ elements for eight slabs are requested together.  D_s = grad_scale_s (G_s - T_s) element by element (G_s is not
// symmetric); exact zeros for a shift with grad_scale_s == 0.  The workgroup's share of loss_scale_s sum (G_s - T_s)^2 is one partial sum of
// the call's ledger record (scale 1): S x pairs x 16 / FQ partial sums, a fixed order, no atomics.  The host takes the smallest FQ of 1, 2,
// 4 whose partial sums fit the record (gs_finish_split): four shifts of 512 channels take FQ = 1 (4096 sums), sixteen FQ = 4.
struct GsTerms {  // launch argument: the host coefficient arrays of one maua_shift_gram_fwd_mse_ledger call
    double loss[GS_SMAX], grad[GS_SMAX];
};
constexpr int GS_FQ_MAX = 4;  // most elements per thread: 16 / 4 workgroups per (shift, tile pair)
template <int FQ>
__global__ void __launch_bounds__(256)
gs_finish_mse_kernel(const float* __restrict__ partial, float* __restrict__ gram, GsShifts sh, GsTerms tw, int C, int npairs, int ksplit,
                     const float* __restrict__ target, float* __restrict__ dmat, double* __restrict__ rec) {
    __shared__ double scratch[16];
    const int s = blockIdx.z;
    const int ntile = (C + GS_T - 1) / GS_T;
    const int ti = blockIdx.x / ntile, tj = blockIdx.x % ntile;
    const double ls = tw.loss[s];
    const float gs = (float)tw.grad[s];
    const int64_t mat = (int64_t)s * C * C;
    int e[FQ];
    int64_t at[FQ];  // the element's place in its matrix, -1 outside it
    float tg[FQ];
#pragma unroll
    for (int u = 0; u < FQ; ++u) {
        e[u] = (blockIdx.y * FQ + u) * 256 + threadIdx.x;
        const int gi = ti * GS_T + e[u] / GS_T, gj = tj * GS_T + e[u] % GS_T;
        at[u] = (gi < C && gj < C) ? mat + (int64_t)gi * C + gj : -1;
        tg[u] = at[u] >= 0 ? target[at[u]] : 0.f;
    }
    const float* base = partial + ((int64_t)s * npairs + blockIdx.x) * ksplit * (GS_T * GS_T);
    double sd[FQ];
#pragma unroll
    for (int u = 0; u < FQ; ++u) sd[u] = 0.0;
    int k = 0;
    for (; k + 7 < ksplit; k += 8) {  // 8 FQ loads in flight, each element's additions in the order of a plain loop
        float v[FQ][8];
#pragma unroll
        for (int u = 0; u < FQ; ++u)
#pragma unroll
            for (int w = 0; w < 8; ++w) v[u][w] = base[(int64_t)(k + w) * (GS_T * GS_T) + e[u]];
#pragma unroll
        for (int u = 0; u < FQ; ++u)
#pragma unroll
            for (int w = 0; w < 8; ++w) sd[u] += (double)v[u][w];
    }
    for (; k < ksplit; ++k) {
        float v[FQ];
#pragma unroll
        for (int u = 0; u < FQ; ++u) v[u] = base[(int64_t)k * (GS_T * GS_T) + e[u]];
#pragma unroll
        for (int u = 0; u < FQ; ++u) sd[u] += (double)v[u];
    }
    double sq = 0.0;
#pragma unroll
    for (int u = 0; u < FQ; ++u) {
        if (at[u] < 0) continue;
        const float g = (float)(sd[u] * sh.factor[s]);
        const float d = g - tg[u];
        gram[at[u]] = g;
        dmat[at[u]] = gs != 0.f ? gs * d : 0.f;
        if (ls != 0.0) sq += (double)d * (double)d;
    }
    sq = block_sum(sq, scratch);
    if (threadIdx.x == 0) {
        rec[2 + ((int64_t)s * npairs + blockIdx.x) * gridDim.y + blockIdx.y] = ls != 0.0 ? sq * ls : 0.0;
        if (blockIdx.x == 0 && blockIdx.y == 0 && s == 0) {
            rec[0] = (double)(gridDim.x * gridDim.y * gridDim.z);
            rec[1] = 1.0;
        }
    }
}

// Backward.  Workgroup = 64 output channels x 256 pixels, wave = 64 x 64 (2 x 2 accumulators), 32 input channels per LDS stage,
// double-buffered (80 KB); the stages run over (shift, term, channel block): term 0 is D_s^T against X at q - off_s, term 1 D_s against X
// at q + off_s.  A (shift, term) whose mask is empty over the workgroup's 256 pixels is left out.
constexpr int GSB_KC = 32, GSB_PX = 256, GSB_CO = 64;

// MASK: the sums (and what they were accumulated into) are written as 0 where relu_mask[c][p] <= 0 (gram_bwd_kernel's pre-masked gradients).
template <bool ACC, bool MASK>
__global__ void __launch_bounds__(256)
gs_bwd_kernel(const float* __restrict__ d, const float* __restrict__ f, const float* __restrict__ mean, const float* __restrict__ relu_mask,
              float* __restrict__ gx, GsShifts sh, int S, int C, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[32][256] + Wl[32][64])
    float* smem = smem_f32;
    constexpr int BUF = GSB_KC * GSB_PX + GSB_KC * GSB_CO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * GSB_PX;
    const int co0 = blockIdx.y * GSB_CO;
    const int64_t pq = p0 + 4 * (tid & 63);  // this thread's pixel quad in every stage (each wave's 64 lanes cover the 256 pixels)

    // the quad's mask for stage run st = 2 s + term, from indices alone
    auto mask_of = [&](int st) -> unsigned {
        const int s = st >> 1, axis = sh.axis[s], delta = sh.delta[s];
        if (st & 1) {  // X at q + off: q itself starts a pair
            return axis == 0 ? gs_mask4(pq, 0, HW, true, W, 0, W - delta) : gs_mask4(pq, 0, (int64_t)(H - delta) * W, false, W, 0, 0);
        }
        return axis == 0 ? gs_mask4(pq, 0, HW, true, W, delta, W) : gs_mask4(pq, (int64_t)delta * W, HW, false, W, 0, 0);
    };
    unsigned active = 0;  // (the same answer in every wave)
    for (int st = 0; st < 2 * S; ++st)
        if (__builtin_amdgcn_ballot_w64(mask_of(st) != 0u) != 0ull && sh.factor[st >> 1] != 0.0) active |= 1u << st;

    f32x4 rx[8], rw[2];
    int loaded_term = 0;
    auto load_stage = [&](int st, int k0) {
        const int s = st >> 1, term = st & 1;
        const int64_t off = sh.axis[s] == 0 ? (int64_t)sh.delta[s] : (int64_t)sh.delta[s] * W;
        const unsigned m = mask_of(st);
        const float cf = (float)sh.factor[s];
        const float* dr = d + (int64_t)s * C * C;
        const int64_t src = term ? pq + off : pq - off;  // used under the mask only
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = k0 + (tid >> 6) + 4 * i;  // quad index tid + 256 i: 32 rows x 64 quads
            const bool in = row < C;
            rx[i] = gs_load4(f + (int64_t)(in ? row : 0) * HW, src, in ? m : 0u, (mean && in) ? mean[row] : 0.f) * cf;
        }
        if (term) {  // Wl[k][co] = D[k0 + k][co0 + co]: rows of D
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + 256 * i;  // 32 rows x 16 quads
                const int row = k0 + (e >> 4), q = e & 15;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = gs_load4_end(dr + (int64_t)row * C, co0 + 4 * q, C);
                rw[i] = v;
            }
        } else {  // Wl[k][co] = D[co0 + co][k0 + k]: quads along k of the rows co, written to LDS transposed
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + 256 * i;  // 64 rows x 8 quads; a wave's lanes hold 64 different rows: conflict-free LDS columns
                const int row = co0 + (e & 63), q = e >> 6;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = gs_load4_end(dr + (int64_t)row * C, k0 + 4 * q, C);
                rw[i] = v;
            }
        }
        loaded_term = term;
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* wl = xl + GSB_KC * GSB_PX;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(xl + (tid + 256 * i) * 4) = rx[i];
        if (loaded_term) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(wl + (tid + 256 * i) * 4) = rw[i];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + 256 * i;
#pragma unroll
                for (int k = 0; k < 4; ++k) wl[(4 * (e >> 6) + k) * GSB_CO + (e & 63)] = rw[i][k];
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

    // the stage to load next: (run st, channel block k0); st == 2 S: none left
    const int NST = 2 * S;
    int st = 0, k0 = 0;
    while (st < NST && !((active >> st) & 1u)) ++st;
    auto advance = [&]() {
        k0 += GSB_KC;
        if (k0 >= C) {
            k0 = 0;
            ++st;
            while (st < NST && !((active >> st) & 1u)) ++st;
        }
    };
    if (st < NST) {  // workgroup-uniform, as every branch on st below
        load_stage(st, k0);
        store_stage(0);
        advance();
        __syncthreads();
        int cur = 0;
        while (true) {
            const bool more = st < NST;
            if (more) load_stage(st, k0);
            const float* xl = smem + cur * BUF;
            const float* wl = xl + GSB_KC * GSB_PX;
#pragma unroll
            for (int kp = 0; kp < GSB_KC / 2; ++kp) {
                const int kk = 2 * kp + half;
                float a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = wl[kk * GSB_CO + t * 32 + j];
#pragma unroll
                for (int u = 0; u < 2; ++u) b[u] = xl[kk * GSB_PX + (wave * 2 + u) * 32 + j];
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

// slabs per (shift, tile pair) and their length in pixels: about 768 workgroups per shift's matrix, slices of whole stages - a function of
// (C, H W) alone
static void gs_plan(int c, int64_t hw, int* npairs, int* ksplit, int64_t* chunk) {
    const int ntile = (c + GS_T - 1) / GS_T;
    *npairs = ntile * ntile;
    const int64_t stages = (hw + GS_K - 1) / GS_K;
    int64_t want = (768 + *npairs - 1) / *npairs;
    if (want > GS_KMAX) want = GS_KMAX;
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    const int64_t ch = ((hw + want - 1) / want + GS_K - 1) / GS_K * GS_K;
    *chunk = ch;
    *ksplit = (int)((hw + ch - 1) / ch);
}

// elements per thread of gs_finish_mse_kernel: the smallest of 1, 2, 4 for which shifts x pairs x 16 / FQ partial sums fit one ledger record
// (0: not even GS_FQ_MAX does)
static int gs_finish_split(int shifts, int64_t npairs) {
    for (int fq = 1; fq <= GS_FQ_MAX; fq *= 2)
        if ((int64_t)shifts * npairs * (GS_T * GS_T / 256 / fq) <= LEDGER_MAX) return fq;
    return 0;
}

static bool gs_shape_ok(int shifts, int c, int h, int w) {
    return shifts >= 1 && shifts <= GS_SMAX && c >= 1 && c <= (1 << 16) && h >= 1 && w >= 1 && (int64_t)h * w < (1ll << 30);
}

// the host arrays of a call into a launch argument; 0, or the error code after set_error
static int gs_pack(const char* who, const int* axes, const int* deltas, const double* factors, int shifts, int h, int w, GsShifts* out) {
    for (int s = 0; s < GS_SMAX; ++s) {
        out->axis[s] = 0;
        out->delta[s] = 1;
        out->factor[s] = 0.0;
    }
    for (int s = 0; s < shifts; ++s) {
        MAUA_REQUIRE(axes[s] == 0 || axes[s] == 1, MAUA_E_UNSUPPORTED, "%s: axis %d of shift %d (0 = x, 1 = y)", who, axes[s], s);
        const int extent = axes[s] == 0 ? w : h;
        MAUA_REQUIRE(deltas[s] >= 1 && deltas[s] < extent, MAUA_E_UNSUPPORTED, "%s: shift %d by %d along an axis of %d (1 .. %d)", who, s,
                     deltas[s], extent, extent - 1);
        out->axis[s] = axes[s];
        out->delta[s] = deltas[s];
        out->factor[s] = factors[s];
    }
    return MAUA_OK;
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_gram_shift_supported(int shifts, int c, int h, int w) { return gs_shape_ok(shifts, c, h, w) ? 1 : 0; }

size_t maua_gram_shift_workspace_bytes(int shifts, int c, int h, int w) {
    if (!gs_shape_ok(shifts, c, h, w)) return 0;
    int npairs, ksplit;
    int64_t chunk;
    gs_plan(c, (int64_t)h * w, &npairs, &ksplit, &chunk);
    return (size_t)shifts * npairs * ksplit * GS_T * GS_T * sizeof(float);
}

// maua_gram_shift_fwd; with `mse` the finishing launch is gs_finish_mse_kernel
struct ShiftMse {
    const float* target;
    const double *loss_scales, *grad_scales;
    float* dmat;
    double* rec;
};
static int gs_forward(const char* who, const float* f, const float* mean, const int* axes, const int* deltas, const double* scales, float* gram,
                      int shifts, int c, int h, int w, void* workspace, size_t workspace_bytes, const ShiftMse* mse, maua_stream_t stream) {
    MAUA_REQUIRE(f && axes && deltas && scales && gram && workspace, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(gs_shape_ok(shifts, c, h, w), MAUA_E_UNSUPPORTED, "%s: %d shifts (1 .. %d), %d channels, %d x %d pixels", who, shifts, GS_SMAX, c,
                 h, w);
    GsShifts sh;
    int rc = gs_pack(who, axes, deltas, scales, shifts, h, w, &sh);
    if (rc) return rc;
    MAUA_REQUIRE(!mse || maua_shift_gram_mse_ledger_supported(shifts, c), MAUA_E_UNSUPPORTED,
                 "%s: %d shifts of %d channels need more than %d partial sums", who, shifts, c, LEDGER_MAX);
    const size_t need = maua_gram_shift_workspace_bytes(shifts, c, h, w);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    int npairs, ksplit;
    int64_t chunk;
    gs_plan(c, (int64_t)h * w, &npairs, &ksplit, &chunk);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gs_partial_kernel, dim3(npairs, ksplit, shifts), dim3(256), 0, s, f, mean, (float*)workspace, sh, c, h, w, npairs, ksplit,
                       chunk);
    rc = check_launch("gs_partial_kernel");
    if (rc) return rc;
    if (mse) {
        GsTerms tw;
        for (int i = 0; i < GS_SMAX; ++i) {
            tw.loss[i] = i < shifts ? mse->loss_scales[i] : 0.0;
            tw.grad[i] = i < shifts ? mse->grad_scales[i] : 0.0;
        }
        const int fq = gs_finish_split(shifts, npairs);
        auto finish = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(npairs, GS_T * GS_T / 256 / fq, shifts), dim3(256), 0, s, (const float*)workspace, gram, sh, tw, c, npairs,
                               ksplit, mse->target, mse->dmat, mse->rec);
        };
        if (fq == 1) finish(gs_finish_mse_kernel<1>);
        else if (fq == 2) finish(gs_finish_mse_kernel<2>);
        else finish(gs_finish_mse_kernel<4>);
        return check_launch("gs_finish_mse_kernel");
    }
    hipLaunchKernelGGL(gs_finish_kernel, dim3(npairs, GS_T * GS_T / 256, shifts), dim3(256), 0, s, (const float*)workspace, gram, sh, c, npairs,
                       ksplit);
    return check_launch("gs_finish_kernel");
}

static int gs_backward(const char* who, const float* d, const float* f, const float* mean, const int* axes, const int* deltas, const double* coefs,
                       const float* relu_mask, float* gx, int shifts, int c, int h, int w, int accumulate, maua_stream_t stream) {
    MAUA_REQUIRE(d && f && axes && deltas && coefs && gx, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(gs_shape_ok(shifts, c, h, w), MAUA_E_UNSUPPORTED, "%s: %d shifts (1 .. %d), %d channels, %d x %d pixels", who, shifts, GS_SMAX, c,
                 h, w);
    GsShifts sh;
    const int rc = gs_pack(who, axes, deltas, coefs, shifts, h, w, &sh);
    if (rc) return rc;
    const int64_t hw = (int64_t)h * w;
    constexpr size_t lds = 2ull * (GSB_KC * GSB_PX + GSB_KC * GSB_CO) * sizeof(float);
    const dim3 grid((unsigned)((hw + GSB_PX - 1) / GSB_PX), (unsigned)((c + GSB_CO - 1) / GSB_CO));
    auto launch = [&](auto kernel) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, d, f, mean, relu_mask, gx, sh, shifts, c, h, w);
    };
    if (relu_mask) {
        if (accumulate) launch(gs_bwd_kernel<true, true>);
        else launch(gs_bwd_kernel<false, true>);
    } else {
        if (accumulate) launch(gs_bwd_kernel<true, false>);
        else launch(gs_bwd_kernel<false, false>);
    }
    return check_launch("gs_bwd_kernel");
}

int maua_gram_shift_fwd(const float* f, const float* mean, const int* axes, const int* deltas, const double* scales, float* gram, int shifts,
                        int c, int h, int w, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    return gs_forward("gram_shift_fwd", f, mean, axes, deltas, scales, gram, shifts, c, h, w, workspace, workspace_bytes, nullptr, stream);
}

int maua_gram_shift_bwd(const float* d, const float* f, const float* mean, const int* axes, const int* deltas, const double* coefs, float* gx,
                        int shifts, int c, int h, int w, int accumulate, maua_stream_t stream) {
    return gs_backward("gram_shift_bwd", d, f, mean, axes, deltas, coefs, nullptr, gx, shifts, c, h, w, accumulate, stream);
}

int maua_shift_gram_mse_ledger_supported(int shifts, int c) {
    if (!gs_shape_ok(shifts, c, 1, 1)) return 0;
    const int64_t nt = (c + GS_T - 1) / GS_T;
    return gs_finish_split(shifts, nt * nt) != 0 ? 1 : 0;
}

int maua_shift_gram_fwd_mse_ledger(const float* f, const float* mean, const int* axes, const int* deltas, const double* scales, float* gram,
                                   int shifts, int c, int h, int w, const float* target, const double* loss_scales, const double* grad_scales,
                                   float* dmat, double* ledger, int slot, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(target && loss_scales && grad_scales && dmat && ledger && slot >= 0 && slot < (1 << 28), MAUA_E_INVAL,
                 "shift_gram_fwd_mse_ledger: bad args");
    const ShiftMse m{target, loss_scales, grad_scales, dmat, ledger + (int64_t)slot * LEDGER_STRIDE};
    return gs_forward("shift_gram_fwd_mse_ledger", f, mean, axes, deltas, scales, gram, shifts, c, h, w, workspace, workspace_bytes, &m, stream);
}

int maua_shift_gram_bwd_masked(const float* d, const float* f, const float* mean, const int* axes, const int* deltas, const double* coefs,
                               const float* relu_mask, float* gx, int shifts, int c, int h, int w, int accumulate, maua_stream_t stream) {
    return gs_backward("shift_gram_bwd_masked", d, f, mean, axes, deltas, coefs, relu_mask, gx, shifts, c, h, w, accumulate, stream);
}

}  // extern "C"
