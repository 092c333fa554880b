// Feature-histogram style loss (Risser, Wilmot & Barnes 2017): every channel of a style layer's activation F[C][N] (N = H W) is
// histogram-matched to the style's channel, given as a quantile table T[C][K] (non-decreasing along k), and the mean squared distance to
// the matched map R is the term; R is a constant in the derivative.  Per channel c, with NB bins:
//     lo = min F[c], hi = max F[c]                                                     exact
//     inv = (float)((double)NB / ((double)hi - (double)lo)), 0 where hi == lo          one fp64 division, rounded once
//     t = fl32(fl32(v - lo) * inv),  b = min(NB - 1, (int)t),  frac = min(1, fl32(t - b))   the decision: no contraction
//     cnt[b] = elements of bin b, cum = its exclusive prefix sum, cum[NB] = N          integers
//     q = (cum[b] + frac cnt[b]) / N,  p = clamp(q K - 0.5, 0, K - 1),  i0 = min(K - 2, floor(p))
//     R = T[c][i0] + (p - i0) (T[c][i0 + 1] - T[c][i0])                                fp32, continuous in its inputs
//     h = sum (F - R)^2 / (C N),   dh/dF = 2 (F - R) / (C N)
// Launch plan.  The grid of every streaming kernel runs over (channel, chunk), flattened: a channel's plane is cut into `chunks` pieces of
// `chunk` elements, a multiple of 1024 (one 16-byte quad per thread), so that about 2048 workgroups of 256 threads run (fh_plan: a function
// of (C, N) alone; C = 64, N = 2^20: 32 chunks of 32768; C = 512, N = 4096: 4 chunks of 1024).
//   forward   fh_range_kernel   reads F: per-workgroup minimum and maximum to workspace slabs; chunk 0 of a channel zeroes its counters
//             fh_count_kernel   reads F: folds the channel's slabs (min / max are exact, any order), counts into an LDS histogram with
//                               integer atomics and adds the non-empty bins to the channel's counters in `state` with integer global atomics
//             fh_scan_kernel    one workgroup per channel: counters -> exclusive prefix sum in place, cum[NB] = N, lo and hi
//             fh_resid_kernel   reads F: T_c and cum_c staged in LDS once, the workgroup's sum of (F - R)^2 in fp64 to the workspace
//             fh_finish_kernel  one workgroup adds the C x chunks partial sums in a fixed order (fp64) and writes loss[0]
//   backward  fh_bwd_kernel     reads F once, writes gx once (read-modify-write when accumulating); R recomputed from `state`
// Integer counts make the merge independent of the order in which workgroups arrive; nothing here uses a float atomic, and the same inputs
// give the same bits.  A ReLU map holds a large share of exact zeros, all of them in bin 0: a wave counts its bin-0 lanes with one ballot
// and one LDS add instead of up to 64 adds to one address.
// Memory accesses are 16 bytes wide where the chunk's first element allows: a scalar head up to the first 16-byte boundary, quads, a scalar
// tail.  An index is compared with the chunk's length before its address is formed.
// The plan, the sweep, the bin arithmetic and the forward kernels live in feat_hist.hpp, which csrc/swd.hip includes as well.
// No packed fp32 instructions: these launches run inside an evaluation, where another stream may issue MFMAs (build_native._file_flags).
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include "feat_hist.hpp"

namespace maua {

template <bool ACC>
__global__ void __launch_bounds__(FH_THREADS)
fh_bwd_kernel(const float* __restrict__ f, const float* __restrict__ table, const int* __restrict__ state, const float* __restrict__ upstream,
              double coef, float* __restrict__ gx, int N, int chunks, int chunk, int bins, int knots) {
    __shared__ float tab[FH_KNOTS_MAX];
    __shared__ int cum[FH_BINS_MAX + 1];
    const int c = blockIdx.x / chunks, ks = blockIdx.x - c * chunks;
    const int p0 = ks * chunk;
    const int n = min(chunk, N - p0);
    float lo, inv;
    fh_stage(table, state, c, bins, knots, tab, cum, &lo, &inv);
    const float nf = (float)N;
    const float s = (float)(coef * (upstream ? (double)upstream[0] : 1.0));
    const float* src = f + (int64_t)c * N + p0;
    float* dst = gx + (int64_t)c * N + p0;
    // quads only where F and gx reach a 16-byte boundary at the same element
    const bool vec = ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    auto value = [&](float v) { return s * (v - fh_match(v, lo, inv, bins, knots, nf, cum, tab)); };
    auto op1 = [&](int i, float v) {
        const float g = value(v);
        dst[i] = ACC ? dst[i] + g : g;
    };
    auto op4 = [&](int i, fh_f32x4 v) {
        fh_f32x4* d4 = reinterpret_cast<fh_f32x4*>(dst + i);
        fh_f32x4 g;
        if constexpr (ACC) g = *d4;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = ACC ? g[k] + value(v[k]) : value(v[k]);
        *d4 = g;
    };
    fh_sweep(src, n, vec, op1, op4);
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_feat_hist_supported(int c, int h, int w, int bins, int knots) { return fh_shape_ok(c, h, w, bins, knots) ? 1 : 0; }

size_t maua_feat_hist_workspace_bytes(int c, int h, int w, int bins, int knots) {
    if (!fh_shape_ok(c, h, w, bins, knots)) return 0;
    int chunks, chunk;
    fh_plan(c, (int64_t)h * w, &chunks, &chunk);
    return (size_t)c * chunks * (sizeof(double) + 2 * sizeof(float));  // partial sums, then the range slabs
}

size_t maua_feat_hist_state_bytes(int c, int bins) {
    if (c < 1 || c > (1 << 16) || bins < FH_BINS_MIN || bins > FH_BINS_MAX) return 0;
    return (size_t)c * (bins + 3) * 4;
}

int maua_feat_hist_fwd(const float* f, const float* table, void* state, float* loss, int c, int h, int w, int bins, int knots, void* workspace,
                       size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(f && table && state && loss && workspace, MAUA_E_INVAL, "feat_hist_fwd: null pointer");
    MAUA_REQUIRE(fh_shape_ok(c, h, w, bins, knots), MAUA_E_UNSUPPORTED,
                 "feat_hist_fwd: %d channels (1 .. 65536), %d x %d pixels (below 2^30), %d bins (%d .. %d), %d knots (%d .. %d)", c, h, w, bins,
                 FH_BINS_MIN, FH_BINS_MAX, knots, FH_KNOTS_MIN, FH_KNOTS_MAX);
    const size_t need = maua_feat_hist_workspace_bytes(c, h, w, bins, knots);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "feat_hist_fwd: workspace %zu < %zu", workspace_bytes, need);
    MAUA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL,
                 "feat_hist_fwd: workspace (8 bytes) or state (4 bytes) misaligned");
    const int N = h * w;
    int chunks, chunk;
    fh_plan(c, N, &chunks, &chunk);
    double* partial = (double*)workspace;
    float* minmax = (float*)(partial + (size_t)c * chunks);
    int* st = (int*)state;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)c * (unsigned)chunks), block(FH_THREADS);  // at most 65536 + 2048
    hipLaunchKernelGGL(fh_range_kernel, grid, block, 0, s, f, st, minmax, N, chunks, chunk, bins);
    int rc = check_launch("fh_range_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_count_kernel, grid, block, 0, s, f, st, (const float*)minmax, N, chunks, chunk, bins, chunks);
    rc = check_launch("fh_count_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_scan_kernel, dim3(c), block, 0, s, st, (const float*)minmax, chunks, bins);
    rc = check_launch("fh_scan_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_resid_kernel, grid, block, 0, s, f, table, (const int*)st, partial, N, chunks, chunk, bins, knots);
    rc = check_launch("fh_resid_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(fh_finish_kernel, dim3(1), block, 0, s, (const double*)partial, c * chunks, 1.0 / ((double)c * (double)N), loss);
    return check_launch("fh_finish_kernel");
}

int maua_feat_hist_bwd(const float* f, const float* table, const void* state, const float* upstream, double coef, float* gx, int c, int h, int w,
                       int bins, int knots, int accumulate, maua_stream_t stream) {
    MAUA_REQUIRE(f && table && state && gx, MAUA_E_INVAL, "feat_hist_bwd: null pointer");
    MAUA_REQUIRE(fh_shape_ok(c, h, w, bins, knots), MAUA_E_UNSUPPORTED,
                 "feat_hist_bwd: %d channels (1 .. 65536), %d x %d pixels (below 2^30), %d bins (%d .. %d), %d knots (%d .. %d)", c, h, w, bins,
                 FH_BINS_MIN, FH_BINS_MAX, knots, FH_KNOTS_MIN, FH_KNOTS_MAX);
    MAUA_REQUIRE((reinterpret_cast<uintptr_t>(state) & 3u) == 0, MAUA_E_INVAL, "feat_hist_bwd: state misaligned");
    const int N = h * w;
    int chunks, chunk;
    fh_plan(c, N, &chunks, &chunk);
    const dim3 grid((unsigned)c * (unsigned)chunks), block(FH_THREADS);  // at most 65536 + 2048
    hipStream_t s = (hipStream_t)stream;
    if (accumulate)
        hipLaunchKernelGGL(fh_bwd_kernel<true>, grid, block, 0, s, f, table, (const int*)state, upstream, coef, gx, N, chunks, chunk, bins, knots);
    else
        hipLaunchKernelGGL(fh_bwd_kernel<false>, grid, block, 0, s, f, table, (const int*)state, upstream, coef, gx, N, chunks, chunk, bins, knots);
    return check_launch("fh_bwd_kernel");
}

}  // extern "C"
