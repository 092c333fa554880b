// Shifted Gram matrices (Berger & Memisevic 2016, "Incorporating long-range consistency in CNN-based texture generation"): for S
// translations (axis_s, delta_s) of one style layer with activation F[C][H W], X = F - mu (mu: the map's row means in the covariance form,
// else 0) and flat pixel index p = y W + x
//     G_s[c][k] = scale_s sum_{p valid for s} X[c][p + off_s] X[k][p]
// off_s = delta_s, valid: x < W - delta_s (axis 0);  off_s = delta_s W, valid: p < (H - delta_s) W (axis 1).  G_s is NOT symmetric.
// Backward, D_s = dL/dG_s as given (not symmetrised):
//     gx[c][q] (+)= sum_s coef_s ( [q - off_s valid] sum_k D_s[c][k] X[k][q - off_s] + [q valid] sum_k D_s[k][c] X[k][q + off_s] ).
//
// The tiles, slabs, fp64 fold, ledger record and backward pipeline are gram_terms.hpp's.  What this file plugs in:
// Forward: ALL tile pairs (G_s is not symmetric), the shift as the term.  A stage's operands are X at p + off_s and X at p, with zeros
// where the pair is invalid, and a slice ends where no pixel starts a pair any more.  The finishing kernels write element by element.
// Backward: every shift gives two runs of stages of one accumulation, D_s^T against X read at q - off_s and D_s against X read at
// q + off_s.  D_s^T is D_s written to LDS transposed, never to memory.
// No load leaves F: the validity mask of a pixel quad is computed from indices first and decides which addresses are formed at all.
// For the fused engine: a finishing kernel that also forms D_s = grad_scale_s (G_s - T_s) and the shifts' loss as one ledger record
// (gs_finish_mse_kernel), and a ReLU mask in the backward kernel's epilogue (gs_bwd_kernel's MASK flag).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include "gram_terms.hpp"

namespace maua {

constexpr int GS_SMAX = 16;   // most shifts per call
constexpr int GS_KMAX = 256;  // most slabs per (shift, tile pair)

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

// One workgroup = one shift x one 64x64 tile pair (ti: rows of G, the operand read at p + off; tj: columns, read at p) x one slice of the
// plane.
__global__ void __launch_bounds__(256)
gs_partial_kernel(const float* __restrict__ f, const float* __restrict__ mean, float* __restrict__ partial, GsShifts sh, int C, int H, int W,
                  int npairs, int ksplit, int64_t chunk) {
    __shared__ __attribute__((aligned(16))) float At[GT_T * GT_RS];
    __shared__ __attribute__((aligned(16))) float Bt[GT_T * GT_RS];
    const int s = blockIdx.z;
    const int tid = threadIdx.x;
    const int ntile = (C + GT_T - 1) / GT_T;
    const int ti = blockIdx.x / ntile, tj = blockIdx.x % ntile;
    const int ks = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const int axis = sh.axis[s], delta = sh.delta[s];
    const int64_t off = axis == 0 ? (int64_t)delta : (int64_t)delta * W;
    const int64_t vend = axis == 0 ? HW : (int64_t)(H - delta) * W;  // pairs start below vend
    const int64_t p_begin = (int64_t)ks * chunk;
    const int64_t p_end = min(min(HW, p_begin + chunk), vend);

    constexpr int NL = GT_T * GT_K / 4 / 256;
    const int r0 = tid >> 4, c4 = (tid & 15) * 4;
    float ma[NL], mb[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int rowa = ti * GT_T + r0 + 16 * q, rowb = tj * GT_T + r0 + 16 * q;
        ma[q] = (mean && rowa < C) ? mean[rowa] : 0.f;
        mb[q] = (mean && rowb < C) ? mean[rowb] : 0.f;
    }
    f32x4 ra[NL], rb[NL];
    auto load_stage = [&](int64_t p0) {
        const int64_t pp = p0 + c4;
        const unsigned m = gs_mask4(pp, 0, p_end, axis == 0, W, 0, W - delta);  // the pair (p, p + off): decided before any address
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int rowa = ti * GT_T + r0 + 16 * q, rowb = tj * GT_T + r0 + 16 * q;
            ra[q] = gt_load4(f + (int64_t)min(rowa, C - 1) * HW, pp + off, rowa < C ? m : 0u, ma[q]);
            rb[q] = gt_load4(f + (int64_t)min(rowb, C - 1) * HW, pp, rowb < C ? m : 0u, mb[q]);
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            *reinterpret_cast<f32x4*>(At + (r0 + 16 * q) * GT_RS + c4) = ra[q];
            *reinterpret_cast<f32x4*>(Bt + (r0 + 16 * q) * GT_RS + c4) = rb[q];
        }
    };

    f32x16 acc = gt_zero16();
    if (p_begin < p_end) {  // workgroup-uniform
        load_stage(p_begin);
        for (int64_t p0 = p_begin; p0 < p_end; p0 += GT_K) {
            __syncthreads();  // previous stage fully consumed
            store_stage();
            __syncthreads();
            if (p0 + GT_K < p_end) load_stage(p0 + GT_K);
            gt_mma_stage(At, Bt, acc);
        }
    }
    gt_store_slab(partial, s, npairs, ksplit, acc);
}

// grid (tile pairs, 16, S): every thread owns one element of the 64x64 tile, folds its slab values and applies the shift's scale.
__global__ void __launch_bounds__(256)
gs_finish_kernel(const float* __restrict__ partial, float* __restrict__ gram, GsShifts sh, int C, int npairs, int ksplit) {
    const int s = blockIdx.z;
    const int ntile = (C + GT_T - 1) / GT_T;
    const int ti = blockIdx.x / ntile, tj = blockIdx.x % ntile;
    const int e[1] = {(int)(blockIdx.y * 256 + threadIdx.x)};
    double sd[1];
    gt_fold<8>(gt_slabs(partial, s, npairs, ksplit), e, ksplit, sd);
    const int gi = ti * GT_T + e[0] / GT_T, gj = tj * GT_T + e[0] % GT_T;
    if (gi < C && gj < C) gram[((int64_t)s * C + gi) * C + gj] = (float)(sd[0] * sh.factor[s]);
}

// gs_finish_kernel and the MSE against the shifts' targets in one launch: grid (tile pairs, 16 / FQ, S), every thread owns FQ elements of the
// 64x64 tile (e = 256 (FQ blockIdx.y + u) + tid), folded exactly as gs_finish_kernel folds them (the same bits); the target elements are
// requested first, so they arrive beside the slabs and not behind them.  D_s = grad_scale_s (G_s - T_s) element by element (G_s is not
// symmetric); exact zeros for a shift with grad_scale_s == 0.  The workgroup's share of loss_scale_s sum (G_s - T_s)^2 is one partial sum of
// the call's ledger record: four shifts of 512 channels take FQ = 1 (4096 sums), sixteen FQ = 4.
struct GsTerms {  // launch argument: the host coefficient arrays of one maua_shift_gram_fwd_mse_ledger call
    double loss[GS_SMAX], grad[GS_SMAX];
};
template <int FQ>
__global__ void __launch_bounds__(256)
gs_finish_mse_kernel(const float* __restrict__ partial, float* __restrict__ gram, GsShifts sh, GsTerms tw, int C, int npairs, int ksplit,
                     const float* __restrict__ target, float* __restrict__ dmat, double* __restrict__ rec) {
    const int s = blockIdx.z;
    const int ntile = (C + GT_T - 1) / GT_T;
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
        const int gi = ti * GT_T + e[u] / GT_T, gj = tj * GT_T + e[u] % GT_T;
        at[u] = (gi < C && gj < C) ? mat + (int64_t)gi * C + gj : -1;
        tg[u] = at[u] >= 0 ? target[at[u]] : 0.f;
    }
    double sd[FQ];
    gt_fold<8>(gt_slabs(partial, s, npairs, ksplit), e, ksplit, sd);
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
    gt_ledger_put(sq, s, npairs, rec, [&](double sum) { return ls != 0.0 ? sum * ls : 0.0; });
}

// Backward: the stage runs are st = 2 s + term: term 0 is D_s^T against X at q - off_s, term 1 D_s against X at q + off_s.  A (shift, term)
// whose mask is empty over the workgroup's 256 pixels is left out.
template <bool ACC, bool MASK>
__global__ void __launch_bounds__(256)
gs_bwd_kernel(const float* __restrict__ d, const float* __restrict__ f, const float* __restrict__ mean, const float* __restrict__ relu_mask,
              float* __restrict__ gx, GsShifts sh, int S, int C, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[32][256] + Wl[32][64])
    float* smem = smem_f32;
    constexpr int BUF = GTB_KC * GTB_PX + GTB_KC * GTB_CO;
    const int tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    const int64_t p0 = (int64_t)blockIdx.x * GTB_PX;
    const int co0 = blockIdx.y * GTB_CO;
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
            rx[i] = gt_load4(f + (int64_t)(in ? row : 0) * HW, src, in ? m : 0u, (mean && in) ? mean[row] : 0.f) * cf;
        }
        if (term) {  // Wl[k][co] = D[k0 + k][co0 + co]: rows of D
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + 256 * i;  // 32 rows x 16 quads
                const int row = k0 + (e >> 4), q = e & 15;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = gt_load4_end(dr + (int64_t)row * C, co0 + 4 * q, C);
                rw[i] = v;
            }
        } else {  // Wl[k][co] = D[co0 + co][k0 + k]: quads along k of the rows co, written to LDS transposed
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = tid + 256 * i;  // 64 rows x 8 quads; a wave's lanes hold 64 different rows: conflict-free LDS columns
                const int row = co0 + (e & 63), q = e >> 6;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < C) v = gt_load4_end(dr + (int64_t)row * C, k0 + 4 * q, C);
                rw[i] = v;
            }
        }
        loaded_term = term;
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* wl = xl + GTB_KC * GTB_PX;
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
                for (int k = 0; k < 4; ++k) wl[(4 * (e >> 6) + k) * GTB_CO + (e & 63)] = rw[i][k];
            }
        }
    };
    gt_bwd_run<ACC, MASK>(smem, active, 2 * S, C, HW, p0, co0, relu_mask, gx, load_stage, store_stage);
}

static bool gs_shape_ok(int shifts, int c, int h, int w) { return h >= 1 && w >= 1 && gt_shape_ok(shifts, GS_SMAX, c, (int64_t)h * w); }

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
    return gt_plan(c, (int64_t)h * w, true, GS_KMAX).slab_bytes(shifts);
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
    const GtPlan p = gt_plan(c, (int64_t)h * w, true, GS_KMAX);
    const size_t need = p.slab_bytes(shifts);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gs_partial_kernel, dim3(p.npairs, p.ksplit, shifts), dim3(256), 0, s, f, mean, (float*)workspace, sh, c, h, w, p.npairs,
                       p.ksplit, p.chunk);
    rc = check_launch("gs_partial_kernel");
    if (rc) return rc;
    if (mse) {
        GsTerms tw;
        for (int i = 0; i < GS_SMAX; ++i) {
            tw.loss[i] = i < shifts ? mse->loss_scales[i] : 0.0;
            tw.grad[i] = i < shifts ? mse->grad_scales[i] : 0.0;
        }
        gt_launch_finish_mse(gs_finish_mse_kernel<1>, gs_finish_mse_kernel<2>, gs_finish_mse_kernel<4>, shifts, p, s, (const float*)workspace, gram,
                             sh, tw, c, p.npairs, p.ksplit, mse->target, mse->dmat, mse->rec);
        return check_launch("gs_finish_mse_kernel");
    }
    hipLaunchKernelGGL(gs_finish_kernel, dim3(p.npairs, GT_T * GT_T / 256, shifts), dim3(256), 0, s, (const float*)workspace, gram, sh, c, p.npairs,
                       p.ksplit);
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
    gt_launch_bwd(gs_bwd_kernel<false, false>, gs_bwd_kernel<true, false>, gs_bwd_kernel<false, true>, gs_bwd_kernel<true, true>, accumulate != 0,
                  relu_mask != nullptr, c, (int64_t)h * w, (hipStream_t)stream, d, f, mean, relu_mask, gx, sh, shifts, c, h, w);
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
    return gs_shape_ok(shifts, c, 1, 1) && gt_finish_split(shifts, gt_pairs(c, true)) != 0 ? 1 : 0;
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
