// Mirrored Gram matrices (Berger & Memisevic 2016, the symmetry terms): for M mirrors of one style layer with activation F[C][H W], X = F - mu
// (mu: the map's row means in the covariance form, else 0), flat pixel index p = y W + x and the involution sigma_m of the pixel grid
//     kind 0 (LR): (y, W - 1 - x)      kind 1 (UD): (H - 1 - y, x)      kind 2 (point mirror, 180 degrees): p -> H W - 1 - p
//     G_m[c][k] = scale_m sum_p X[c][sigma_m(p)] X[k][p]         over ALL pixels; symmetric, and returned bit-symmetric.
// Backward, D_m = dL/dG_m as given (not symmetrised):
//     gx[c][q] (+)= sum_m coef_m sum_k (D_m[c][k] + D_m[k][c]) X[k][sigma_m(q)].
//
// The tiles, slabs, fp64 fold, ledger record and backward layout are gram_terms.hpp's (gf_bwd_kernel keeps its own text of the backward
// pipeline, for speed: see there).  What this file plugs in:
// Forward: the tile pairs ti <= tj only, the mirror as the term, int pixel indices (H W < 2^30).  A stage's operands are X at sigma(p) and
// X at p, zeros behind the plane's end; the wave below the diagonal of a diagonal tile stages its share but multiplies nothing.  The finishing
// kernels write (i, j) and (j, i) from the same sum - inside a diagonal tile from the triangle er <= ec only, since the two triangles of an
// MFMA tile add their products in different orders.
// Backward: one run of stages per mirror: the weight stage holds D_m[k][co] + D_m[co][k], added in registers before the LDS store.
// The mirrored operand: sigma(p) descends as p ascends (LR, 180), so a pixel quad inside one row is the four consecutive addresses
// sigma(p) - 3 .. sigma(p), one 16-byte load reversed in registers; UD reads whole rows ascending.  A quad that crosses a row end or the plane's
// end goes element by element.  sigma(p) lies inside F exactly when p does: the mask of a quad (p < H W) is computed from indices first and
// decides which addresses are formed at all.
// For the fused engine: a finishing kernel that also forms D_m = grad_scale_m (G_m - T_m) and the mirrors' loss as one ledger record
// (gf_finish_mse_kernel), and a ReLU mask in the backward kernel's epilogue (gf_bwd_kernel's MASK flag).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include "gram_terms.hpp"

namespace maua {

constexpr int GF_MMAX = 4;    // most mirrors per call
constexpr int GF_KMAX = 768;  // most slabs per (mirror, tile pair): a single tile pair (C <= 64) still fills the device

struct GfMirrors {  // launch argument: the host arrays of one call
    int kind[GF_MMAX];
    double factor[GF_MMAX];  // scale_m (forward) / coef_m (backward)
};

// bit k: pixel p + k lies below `end`
__device__ __forceinline__ unsigned gf_mask4(int p, int end) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k < end) m |= 1u << k;
    return m;
}

// row[sigma(p + k)] - mu for the elements k of the mask (all of them below H W), 0 for the others.  (y, x) are the row and column of p.
__device__ __forceinline__ f32x4 gf_load4_mirror(const float* __restrict__ row, int p, unsigned m, float mu, int kind, int H, int W, int y, int x) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int HW = H * W;
    if (m == 15u && (kind == 2 || x + 3 < W)) {  // the whole quad inside the plane and (LR, UD) inside one row: four consecutive addresses
        const int a = kind == 2 ? HW - 4 - p : kind == 0 ? y * W + (W - 4 - x) : (H - 1 - y) * W + x;
        const f32x4 t = *reinterpret_cast<const gt_f32x4u*>(row + a);
        if (kind == 1) {
            v = t;
        } else {
            v[0] = t[3], v[1] = t[2], v[2] = t[1], v[3] = t[0];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] -= mu;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((m >> k) & 1u) {
                const int pk = p + k, yy = pk / W, xx = pk - yy * W;
                const int a = kind == 2 ? HW - 1 - pk : kind == 0 ? yy * W + (W - 1 - xx) : (H - 1 - yy) * W + xx;
                v[k] = row[a] - mu;
            }
    }
    return v;
}

// One workgroup = one mirror x one 64x64 tile pair ti <= tj (ti: rows of G, the operand read at sigma(p); tj: columns, read at p) x one slice
// of the plane.
__global__ void __launch_bounds__(256)
gf_partial_kernel(const float* __restrict__ f, const float* __restrict__ mean, float* __restrict__ partial, GfMirrors mr, int C, int H, int W,
                  int npairs, int ksplit, int chunk) {
    __shared__ __attribute__((aligned(16))) float At[GT_T * GT_RS];
    __shared__ __attribute__((aligned(16))) float Bt[GT_T * GT_RS];
    const int s = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const int ks = blockIdx.y;
    const int HW = H * W;  // below 2^30
    const int kind = mr.kind[s];
    const int p_begin = ks * chunk;  // ks chunk < H W + chunk
    const int p_end = min(HW, p_begin + chunk);

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
    auto load_stage = [&](int p0) {
        const int pp = p0 + c4;
        const unsigned m = gf_mask4(pp, p_end);  // decided before any address
        const int y = pp / W, x = pp - y * W;
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int rowa = ti * GT_T + r0 + 16 * q, rowb = tj * GT_T + r0 + 16 * q;
            ra[q] = gf_load4_mirror(f + (int64_t)min(rowa, C - 1) * HW, pp, rowa < C ? m : 0u, ma[q], kind, H, W, y, x);
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
        for (int p0 = p_begin; p0 < p_end; p0 += GT_K) {
            __syncthreads();  // previous stage fully consumed
            store_stage();
            __syncthreads();
            if (p0 + GT_K < p_end) load_stage(p0 + GT_K);
            if (ti == tj && wi > wj) continue;  // (wave-uniform) the block below the diagonal of a diagonal tile is never read
            gt_mma_stage(At, Bt, acc);
        }
    }
    gt_store_slab(partial, s, npairs, ksplit, acc);
}

// grid (tile pairs, 16, M): every thread owns one element of the 64x64 tile, folds its slab values, applies the mirror's scale and writes
// the element and its transpose; in a diagonal tile the threads with er <= ec only.
__global__ void __launch_bounds__(256)
gf_finish_kernel(const float* __restrict__ partial, float* __restrict__ gram, GfMirrors mr, int C, int npairs, int ksplit) {
    const int s = blockIdx.z;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const int e[1] = {(int)(blockIdx.y * 256 + threadIdx.x)};
    const int er = e[0] / GT_T, ec = e[0] % GT_T;
    const int gi = ti * GT_T + er, gj = tj * GT_T + ec;
    if (gi >= C || gj >= C || (ti == tj && er > ec)) return;
    double sd[1];
    gt_fold<16>(gt_slabs(partial, s, npairs, ksplit), e, ksplit, sd);
    const float g = (float)(sd[0] * mr.factor[s]);
    float* gm = gram + (int64_t)s * C * C;
    gm[(int64_t)gi * C + gj] = g;
    gm[(int64_t)gj * C + gi] = g;
}

// gf_finish_kernel and the MSE against the mirrors' targets in one launch: grid (tile pairs, 16 / FQ, M), every thread owns FQ elements of
// the 64x64 tile (e = 256 (FQ blockIdx.y + u) + tid); in a diagonal tile the elements with er <= ec only are live.  Each live element is
// folded exactly as gf_finish_kernel folds it (the same bits; the other threads fold an element they do not use, which keeps every load
// unconditional); the target elements - read on and above the diagonal only - are requested first, so they arrive beside the slabs and
// not behind them.  D_m = grad_scale_m (G_m - T_m) is formed once per live element and written with its mirror like G_m (bit-symmetric
// whatever the target holds below its diagonal); exact zeros for a mirror with grad_scale_m == 0.  The workgroup's share of loss_scale_m
// sum (G_m - T_m)^2 - an element off the diagonal counts twice - is one partial sum of the call's ledger record: three mirrors of 512
// channels take FQ = 1 (1728 sums).
struct GfTerms {  // launch argument: the host coefficient arrays of one maua_flip_gram_fwd_mse_ledger call
    double loss[GF_MMAX], grad[GF_MMAX];
};
template <int FQ>
__global__ void __launch_bounds__(256)
gf_finish_mse_kernel(const float* __restrict__ partial, float* __restrict__ gram, GfMirrors mr, GfTerms tw, int C, int npairs, int ksplit,
                     const float* __restrict__ target, float* __restrict__ dmat, double* __restrict__ rec) {
    const int s = blockIdx.z;
    int ti, tj;
    gt_pair_upper(blockIdx.x, (C + GT_T - 1) / GT_T, &ti, &tj);
    const double ls = tw.loss[s];
    const float gs = (float)tw.grad[s];
    const int64_t mat = (int64_t)s * C * C;
    int e[FQ], gi[FQ], gj[FQ];
    bool live[FQ];
    float tg[FQ];
#pragma unroll
    for (int u = 0; u < FQ; ++u) {
        e[u] = (blockIdx.y * FQ + u) * 256 + threadIdx.x;
        const int er = e[u] / GT_T, ec = e[u] % GT_T;
        gi[u] = ti * GT_T + er;
        gj[u] = tj * GT_T + ec;
        live[u] = gi[u] < C && gj[u] < C && !(ti == tj && er > ec);
        tg[u] = live[u] ? target[mat + (int64_t)gi[u] * C + gj[u]] : 0.f;
        // every thread folds some element of the slabs, so that the loads below carry no condition and stay in flight together: an element
        // below the diagonal of a diagonal tile folds its row's diagonal element (the cache lines its wave reads anyway; the sum is not used)
        if (ti == tj && er > ec) e[u] = er * GT_T + er;
    }
    double sd[FQ];
    gt_fold<16>(gt_slabs(partial, s, npairs, ksplit), e, ksplit, sd);
    double sq = 0.0;
#pragma unroll
    for (int u = 0; u < FQ; ++u) {
        if (!live[u]) continue;
        const float g = (float)(sd[u] * mr.factor[s]);
        const float d = g - tg[u];
        const float dv = gs != 0.f ? gs * d : 0.f;
        const int64_t up = mat + (int64_t)gi[u] * C + gj[u], low = mat + (int64_t)gj[u] * C + gi[u];
        gram[up] = g;
        gram[low] = g;
        dmat[up] = dv;
        dmat[low] = dv;
        if (ls != 0.0) sq += (gi[u] != gj[u] ? 2.0 : 1.0) * ((double)d * (double)d);
    }
    gt_ledger_put(sq, s, npairs, rec, [&](double sum) { return ls != 0.0 ? sum * ls : 0.0; });
}

// Backward: the stage runs are the mirrors.  A mirror whose coef is 0 is left out.
template <bool ACC, bool MASK>
__global__ void __launch_bounds__(256)
gf_bwd_kernel(const float* __restrict__ d, const float* __restrict__ f, const float* __restrict__ mean, const float* __restrict__ relu_mask,
              float* __restrict__ gx, GfMirrors mr, int M, int C, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float smem_f32[];  // 2 x (Xl[32][256] + Wl[32][64])
    float* smem = smem_f32;
    constexpr int BUF = GTB_KC * GTB_PX + GTB_KC * GTB_CO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const int HW = H * W;
    const int p0 = blockIdx.x * GTB_PX;
    const int co0 = blockIdx.y * GTB_CO;
    const int pq = p0 + 4 * (tid & 63);  // this thread's pixel quad in every stage (each wave's 64 lanes cover the 256 pixels)
    const unsigned mq = gf_mask4(pq, HW);  // from indices alone; sigma(q) lies inside F exactly when q does
    const int qy = pq / W, qx = pq - qy * W;

    unsigned active = 0;
    for (int s = 0; s < M; ++s)
        if (mr.factor[s] != 0.0) active |= 1u << s;

    f32x4 rx[8], rw[2];
    auto load_stage = [&](int s, int k0) {
        const int kind = mr.kind[s];
        const float cf = (float)mr.factor[s];
        const float* dr = d + (int64_t)s * C * C;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = k0 + (tid >> 6) + 4 * i;  // quad index tid + 256 i: 32 rows x 64 quads
            const bool in = row < C;
            rx[i] = gf_load4_mirror(f + (int64_t)(in ? row : 0) * HW, pq, in ? mq : 0u, (mean && in) ? mean[row] : 0.f, kind, H, W, qy, qx) * cf;
        }
        // Wl[k][co] = D[co0 + co][k0 + k] + D[k0 + k][co0 + co]: this thread holds (co, k .. k + 3) - a quad along k of the row co, and four
        // elements of the column co, which a wave's 64 lanes (64 consecutive co) read as whole lines
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i;  // 64 rows x 8 quads
            const int co = co0 + (e & 63), kq = k0 + 4 * (e >> 6);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (co < C) {
                const float* drow = dr + (int64_t)co * C;
                if (kq + 4 <= C) {  // (int indices, as everywhere in this file: gt_load4_end compares in 64 bits)
                    v = *reinterpret_cast<const gt_f32x4u*>(drow + kq);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (kq + k < C) v[k] = drow[kq + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (kq + k < C) v[k] += dr[(int64_t)(kq + k) * C + co];
            }
            rw[i] = v;
        }
    };
    auto store_stage = [&](int buf) {
        float* xl = smem + buf * BUF;
        float* wl = xl + GTB_KC * GTB_PX;
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(xl + (tid + 256 * i) * 4) = rx[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i;  // a wave's lanes hold 64 different co: conflict-free LDS columns
#pragma unroll
            for (int k = 0; k < 4; ++k) wl[(4 * (e >> 6) + k) * GTB_CO + (e & 63)] = rw[i][k];
        }
    };
    // The pipeline and epilogue below are gt_bwd_run's, kept here in this file's own text: built through the shared template this kernel
    // alone came out 2 - 7 % slower (profiles/refactor_gram_terms.md), with the same registers and MFMAs and a different schedule.
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

    // the stage to load next: (mirror st, channel block k0); st == M: none left
    int st = 0, k0 = 0;
    while (st < M && !((active >> st) & 1u)) ++st;
    auto advance = [&]() {
        k0 += GTB_KC;
        if (k0 >= C) {
            k0 = 0;
            ++st;
            while (st < M && !((active >> st) & 1u)) ++st;
        }
    };
    if (st < M) {  // workgroup-uniform, as every branch on st below
        load_stage(st, k0);
        store_stage(0);
        advance();
        __syncthreads();
        int cur = 0;
        while (true) {
            const bool more = st < M;
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
        const int pix = p0 + (wave * 2 + u) * 32 + j;
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

static bool gf_shape_ok(int mirrors, int c, int h, int w) { return h >= 1 && w >= 1 && gt_shape_ok(mirrors, GF_MMAX, c, (int64_t)h * w); }

// the host arrays of a call into a launch argument; 0, or the error code after set_error
static int gf_pack(const char* who, const int* kinds, const double* factors, int mirrors, GfMirrors* out) {
    for (int s = 0; s < GF_MMAX; ++s) {
        out->kind[s] = 0;
        out->factor[s] = 0.0;
    }
    for (int s = 0; s < mirrors; ++s) {
        MAUA_REQUIRE(kinds[s] >= 0 && kinds[s] <= 2, MAUA_E_UNSUPPORTED, "%s: kind %d of mirror %d (0 = LR, 1 = UD, 2 = point mirror)", who,
                     kinds[s], s);
        out->kind[s] = kinds[s];
        out->factor[s] = factors[s];
    }
    return MAUA_OK;
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_gram_flip_supported(int mirrors, int c, int h, int w) { return gf_shape_ok(mirrors, c, h, w) ? 1 : 0; }

size_t maua_gram_flip_workspace_bytes(int mirrors, int c, int h, int w) {
    if (!gf_shape_ok(mirrors, c, h, w)) return 0;
    return gt_plan(c, (int64_t)h * w, false, GF_KMAX).slab_bytes(mirrors);
}

// maua_gram_flip_fwd; with `mse` the finishing launch is gf_finish_mse_kernel
struct FlipMse {
    const float* target;
    const double *loss_scales, *grad_scales;
    float* dmat;
    double* rec;
};
static int gf_forward(const char* who, const float* f, const float* mean, const int* kinds, const double* scales, float* gram, int mirrors, int c,
                      int h, int w, void* workspace, size_t workspace_bytes, const FlipMse* mse, maua_stream_t stream) {
    MAUA_REQUIRE(f && kinds && scales && gram && workspace, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(gf_shape_ok(mirrors, c, h, w), MAUA_E_UNSUPPORTED, "%s: %d mirrors (1 .. %d), %d channels, %d x %d pixels", who, mirrors, GF_MMAX,
                 c, h, w);
    GfMirrors mr;
    int rc = gf_pack(who, kinds, scales, mirrors, &mr);
    if (rc) return rc;
    MAUA_REQUIRE(!mse || maua_flip_gram_mse_ledger_supported(mirrors, c), MAUA_E_UNSUPPORTED,
                 "%s: %d mirrors of %d channels need more than %d partial sums", who, mirrors, c, LEDGER_MAX);
    const GtPlan p = gt_plan(c, (int64_t)h * w, false, GF_KMAX);
    const size_t need = p.slab_bytes(mirrors);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gf_partial_kernel, dim3(p.npairs, p.ksplit, mirrors), dim3(256), 0, s, f, mean, (float*)workspace, mr, c, h, w, p.npairs,
                       p.ksplit, (int)p.chunk);
    rc = check_launch("gf_partial_kernel");
    if (rc) return rc;
    if (mse) {
        GfTerms tw;
        for (int i = 0; i < GF_MMAX; ++i) {
            tw.loss[i] = i < mirrors ? mse->loss_scales[i] : 0.0;
            tw.grad[i] = i < mirrors ? mse->grad_scales[i] : 0.0;
        }
        gt_launch_finish_mse(gf_finish_mse_kernel<1>, gf_finish_mse_kernel<2>, gf_finish_mse_kernel<4>, mirrors, p, s, (const float*)workspace, gram,
                             mr, tw, c, p.npairs, p.ksplit, mse->target, mse->dmat, mse->rec);
        return check_launch("gf_finish_mse_kernel");
    }
    hipLaunchKernelGGL(gf_finish_kernel, dim3(p.npairs, GT_T * GT_T / 256, mirrors), dim3(256), 0, s, (const float*)workspace, gram, mr, c, p.npairs,
                       p.ksplit);
    return check_launch("gf_finish_kernel");
}

static int gf_backward(const char* who, const float* d, const float* f, const float* mean, const int* kinds, const double* coefs,
                       const float* relu_mask, float* gx, int mirrors, int c, int h, int w, int accumulate, maua_stream_t stream) {
    MAUA_REQUIRE(d && f && kinds && coefs && gx, MAUA_E_INVAL, "%s: null pointer", who);
    MAUA_REQUIRE(gf_shape_ok(mirrors, c, h, w), MAUA_E_UNSUPPORTED, "%s: %d mirrors (1 .. %d), %d channels, %d x %d pixels", who, mirrors, GF_MMAX,
                 c, h, w);
    GfMirrors mr;
    const int rc = gf_pack(who, kinds, coefs, mirrors, &mr);
    if (rc) return rc;
    gt_launch_bwd(gf_bwd_kernel<false, false>, gf_bwd_kernel<true, false>, gf_bwd_kernel<false, true>, gf_bwd_kernel<true, true>, accumulate != 0,
                  relu_mask != nullptr, c, (int64_t)h * w, (hipStream_t)stream, d, f, mean, relu_mask, gx, mr, mirrors, c, h, w);
    return check_launch("gf_bwd_kernel");
}

int maua_gram_flip_fwd(const float* f, const float* mean, const int* kinds, const double* scales, float* gram, int mirrors, int c, int h, int w,
                       void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    return gf_forward("gram_flip_fwd", f, mean, kinds, scales, gram, mirrors, c, h, w, workspace, workspace_bytes, nullptr, stream);
}

int maua_gram_flip_bwd(const float* d, const float* f, const float* mean, const int* kinds, const double* coefs, float* gx, int mirrors, int c,
                       int h, int w, int accumulate, maua_stream_t stream) {
    return gf_backward("gram_flip_bwd", d, f, mean, kinds, coefs, nullptr, gx, mirrors, c, h, w, accumulate, stream);
}

int maua_flip_gram_mse_ledger_supported(int mirrors, int c) {
    return gf_shape_ok(mirrors, c, 1, 1) && gt_finish_split(mirrors, gt_pairs(c, false)) != 0 ? 1 : 0;
}

int maua_flip_gram_fwd_mse_ledger(const float* f, const float* mean, const int* kinds, const double* scales, float* gram, int mirrors, int c,
                                  int h, int w, const float* target, const double* loss_scales, const double* grad_scales, float* dmat,
                                  double* ledger, int slot, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(target && loss_scales && grad_scales && dmat && ledger && slot >= 0 && slot < (1 << 28), MAUA_E_INVAL,
                 "flip_gram_fwd_mse_ledger: bad args");
    const FlipMse m{target, loss_scales, grad_scales, dmat, ledger + (int64_t)slot * LEDGER_STRIDE};
    return gf_forward("flip_gram_fwd_mse_ledger", f, mean, kinds, scales, gram, mirrors, c, h, w, workspace, workspace_bytes, &m, stream);
}

int maua_flip_gram_bwd_masked(const float* d, const float* f, const float* mean, const int* kinds, const double* coefs, const float* relu_mask,
                              float* gx, int mirrors, int c, int h, int w, int accumulate, maua_stream_t stream) {
    return gf_backward("flip_gram_bwd_masked", d, f, mean, kinds, coefs, relu_mask, gx, mirrors, c, h, w, accumulate, stream);
}

}  // extern "C"
