// scipy.ndimage.gaussian_filter(np.roll(x, -roll_t, axis=0), [sigma_t, 0, sigma_h, sigma_w], mode="wrap") for a (T, C, H, W) fp32 clip that
// stays in HBM: the initial clip of style.img_vid (sigma = [T, 0, H/32, W/32] or [T, 0, 4, 4]) and the temporal blend between two scales
// (sigma = [temporal_blend, 0, 0, 0] after a roll by 7 frames), plan field clip_device = 1.  The reference only calls scipy here; nothing
// in this file comes from it.
//   * one separable pass per axis with sigma > 1e-15, in scipy's order T, H, W; radius r = int(4 sigma + 0.5); weights
//     exp(-0.5 / sigma^2 * j^2) / sum in fp64; every pass sums in fp64 in a fixed tap order (ascending offset) and rounds to fp32 once.
//   * "wrap" is purely periodic: tap j of output i reads (i + j) mod L.  Where 2 r + 1 > L the taps are folded onto the L residues once
//     (f[d] = sum of w[j] over j = d mod L, ascending j), and the pass runs L taps: a pass never has more taps than its axis has elements.
//   * the weight tables are built on the device, on the stream (gauss_wrap_weights_kernel), into the head of the workspace.
//   * the roll is a frame offset on the read side of the first pass (circular filters commute with it); no pass: two device copies.
//   * passes alternate between y and a clip-sized region of the workspace so that the last one writes y; x is never written.
// Pass kernels: the filtered axis has stride `inner` elements.  inner > 1 (T and H passes): a workgroup stages S rows x 64 columns in LDS,
// lanes along the contiguous columns (global loads coalesced, LDS reads of a wave on 64 neighbouring banks); a thread forms four
// consecutive outputs of its column from one walk over the staged rows.  A tile that would need the whole axis anyway stages the axis
// once and indexes it modulo L; a tile that does not fit LDS reads its taps from global memory (L2 serves the reuse).  inner == 1 (W
// pass): a wave stages one row segment plus its wrapped halo, lanes along the segment, four outputs 64 apart per thread.
// No atomics, no state: reruns are bit-identical.  These kernels run between two optimize calls, possibly beside another stream's MFMA
// kernels, so none may hold packed fp32 instructions (tests/test_abi.py keeps the list of kernels that do closed):
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <math.h>

#include "common.hpp"

namespace maua {

constexpr int GW_MAX_RADIUS = MAUA_GAUSS_WRAP_MAX_RADIUS;
constexpr int GW_LDS_FLOATS = 152 * 1024 / 4;  // strided pass: most LDS a tile takes, of the CU's 160 KiB (above 64 KiB: opt_in_dynamic_lds)
constexpr int GW_COLS = 64;                    // strided pass: columns of a tile = lanes of a wave
constexpr int GW_ROWS_CAP = GW_LDS_FLOATS / GW_COLS;
constexpr int GW_ROW_TILE = 1024;              // W pass: outputs of a tile along the row
constexpr int GW_ROW_LDS_FLOATS = 10240;       // W pass: LDS a workgroup aims at (1 .. 16 rows of R + n - 1 floats)

struct GwAxis {
    double sigma;
    double* tab;  // n weights: tab[k] multiplies element (i + shift + k) mod L
    int r, n, L, folded;
};
struct GwTables {
    GwAxis a[3];
};

// One workgroup per filtered axis.  The normalising sum is formed in a fixed order (strided partial sums, wave shuffles, waves in index order).
__global__ void __launch_bounds__(256) gauss_wrap_weights_kernel(GwTables t) {
    __shared__ double scratch[16];
    __shared__ double total;
    const GwAxis ax = t.a[blockIdx.x];
    if (ax.n <= 0) return;
    const double c = -0.5 / (ax.sigma * ax.sigma);
    double part = 0.0;
    for (int j = -ax.r + (int)threadIdx.x; j <= ax.r; j += 256) part += exp(c * ((double)j * (double)j));
    const double sum = block_sum(part, scratch);
    if (threadIdx.x == 0) total = sum;
    __syncthreads();
    for (int d = threadIdx.x; d < ax.n; d += 256) {
        if (!ax.folded) {
            const double j = (double)(d - ax.r);
            ax.tab[d] = exp(c * (j * j)) / total;
        } else {
            double f = 0.0;
            for (int j = -ax.r + (d + ax.r) % ax.L; j <= ax.r; j += ax.L) f += exp(c * ((double)j * (double)j)) / total;
            ax.tab[d] = f;
        }
    }
}

struct GwPass {
    const float* src;
    float* dst;
    const double* tab;
    int64_t outer, L, inner;  // the clip as [outer][L][inner]
    int n, shift;             // taps; first tap of output i reads (i + shift) mod L (the T pass carries the roll in here)
    int64_t per_frame;        // outer indices per frame (H pass: C, W pass: C * H; T pass: outer = 1)
    int T, roll;              // H / W pass as the first pass: frame t reads frame (t + roll) mod T
    int R, S, whole;          // outputs along L per tile, staged elements along L, 1 = the whole axis is staged and indexed mod L
    int64_t ltiles, ctiles, tiles;
};

__device__ __forceinline__ int64_t gw_src_outer(const GwPass& p, int64_t q) {
    if (p.roll == 0) return q;
    const int64_t t = q / p.per_frame, rest = q - t * p.per_frame;
    return ((t + p.roll) % p.T) * p.per_frame + rest;
}

constexpr int GW_M = 4;  // outputs a thread forms together: consecutive along L (strided pass: one LDS read feeds GW_M sums), 64 apart (row pass)

template <bool EDGE>
__device__ __forceinline__ void gw_slide_step(const double* __restrict__ tab, int n, int s, double v, double (&w)[GW_M], double (&acc)[GW_M]) {
#pragma unroll
    for (int m = GW_M - 1; m > 0; --m) w[m] = w[m - 1];
    w[0] = (!EDGE || s < n) ? tab[s] : 0.0;
#pragma unroll
    for (int m = 0; m < GW_M; ++m)
        if (!EDGE || (s >= m && s - m < n)) acc[m] += w[m] * v;  // (a tap outside the filter is skipped, not multiplied by zero: an infinity stays where scipy leaves it)
}

// GW_M consecutive outputs of one column from a staged axis of S elements: output m sums tab[k] * e[(idx + m + k) mod S] for ascending k.
// Step s reads element idx + s once and feeds tap k = s - m of every output m; w[m] = tab[s - m] moves along with it.
__device__ __forceinline__ void gw_slide(const double* __restrict__ tab, int n, const float* col, int stride, int idx, int S, double (&acc)[GW_M]) {
    double w[GW_M];
#pragma unroll
    for (int m = 0; m < GW_M; ++m) w[m] = 0.0, acc[m] = 0.0;
    const int steps = n + GW_M - 1, lead = GW_M - 1, tail = n > lead ? n : lead;
    int s = 0;
    for (; s < lead; ++s) {
        gw_slide_step<true>(tab, n, s, (double)col[(int64_t)idx * stride], w, acc);
        idx = idx + 1 == S ? 0 : idx + 1;
    }
#pragma unroll 4
    for (; s < n; ++s) {
        gw_slide_step<false>(tab, n, s, (double)col[(int64_t)idx * stride], w, acc);
        idx = idx + 1 == S ? 0 : idx + 1;
    }
    for (s = tail; s < steps; ++s) {
        gw_slide_step<true>(tab, n, s, (double)col[(int64_t)idx * stride], w, acc);
        idx = idx + 1 == S ? 0 : idx + 1;
    }
}

// T and H passes: tile = R outputs along L x 64 columns of `inner`; thread = (column, group of GW_M consecutive rows); blockDim.x / 64 groups.
__global__ void __launch_bounds__(1024) gauss_wrap_strided_kernel(GwPass p) {
    extern __shared__ float gw_lds[];
    const int col = threadIdx.x & 63, rg = threadIdx.x >> 6, groups = blockDim.x >> 6;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t lt = tile % p.ltiles, rest = tile / p.ltiles, ct = rest % p.ctiles, q = rest / p.ctiles;
        const int64_t c = ct * GW_COLS + col, i0 = lt * p.R;
        const bool live = c < p.inner;
        const float* s = p.src + gw_src_outer(p, q) * p.L * p.inner + c;
        const int64_t g0 = p.whole ? 0 : (i0 + p.shift) % p.L;
        for (int r = rg; r < p.S; r += groups) {
            int64_t g = g0 + r;
            g -= g >= p.L ? p.L : 0;
            gw_lds[r * GW_COLS + col] = live ? s[g * p.inner] : 0.f;
        }
        __syncthreads();
        for (int r0 = rg * GW_M; r0 < p.R; r0 += groups * GW_M) {
            if (i0 + r0 >= p.L) break;
            double acc[GW_M];
            gw_slide(p.tab, p.n, gw_lds + col, GW_COLS, p.whole ? (int)((i0 + r0 + p.shift) % p.L) : r0, p.S, acc);
            float* d = p.dst + (q * p.L + i0 + r0) * p.inner + c;
#pragma unroll
            for (int m = 0; m < GW_M; ++m)
                if (live && r0 + m < p.R && i0 + r0 + m < p.L) d[(int64_t)m * p.inner] = (float)acc[m];
        }
        __syncthreads();
    }
}

// W pass (inner == 1): tile = blockDim.x / 64 rows x R outputs along the row; wave = row, lanes along the row.  A wave stages its R outputs'
// elements and the n - 1 behind them (indices mod L: the halo of a short row laps it), so no tap wraps; a thread forms GW_M outputs 64 apart.
__global__ void __launch_bounds__(1024) gauss_wrap_row_kernel(GwPass p) {
    extern __shared__ float gw_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = blockDim.x >> 6;
    float* row = gw_lds + (int64_t)wave * p.S;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int64_t lt = tile % p.ltiles, q = (tile / p.ltiles) * rows + wave, x0 = lt * p.R;
        const bool live = q < p.outer;
        const float* s = p.src + (live ? gw_src_outer(p, q) : 0) * p.L;
        const int64_t g0 = (x0 + p.shift) % p.L;
        for (int e = lane; e < p.S; e += 64) row[e] = live ? s[(g0 + e) % p.L] : 0.f;
        __syncthreads();
        for (int e0 = lane; e0 < p.R; e0 += 64 * GW_M) {
            double acc[GW_M];
            const float* in[GW_M];
#pragma unroll
            for (int m = 0; m < GW_M; ++m) acc[m] = 0.0, in[m] = row + (e0 + 64 * m < p.R ? e0 + 64 * m : e0);  // (a lane past the tile repeats its first output)
#pragma unroll 4
            for (int k = 0; k < p.n; ++k) {
                const double wk = p.tab[k];
#pragma unroll
                for (int m = 0; m < GW_M; ++m) acc[m] += wk * (double)in[m][k];
            }
#pragma unroll
            for (int m = 0; m < GW_M; ++m) {
                const int64_t e = e0 + 64 * m, x = x0 + e;
                if (live && e < p.R && x < p.L) p.dst[q * p.L + x] = (float)acc[m];
            }
        }
        __syncthreads();
    }
}

// A strided pass whose tile does not fit LDS: one thread per output, taps from global memory, consecutive lanes on consecutive columns.
__global__ void __launch_bounds__(256) gauss_wrap_global_kernel(GwPass p) {
    const int64_t total = p.outer * p.L * p.inner;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = e % p.inner, i = (e / p.inner) % p.L, q = e / (p.inner * p.L);
        const float* s = p.src + gw_src_outer(p, q) * p.L * p.inner + c;
        const int64_t idx = (i + p.shift) % p.L;
        const int n1 = p.n < p.L - idx ? p.n : (int)(p.L - idx);
        double acc = 0.0;
#pragma unroll 4
        for (int k = 0; k < n1; ++k) acc += p.tab[k] * (double)s[(idx + k) * p.inner];
#pragma unroll 4
        for (int k = n1; k < p.n; ++k) acc += p.tab[k] * (double)s[(int64_t)(k - n1) * p.inner];
        p.dst[e] = (float)acc;
    }
}

struct GwPlan {
    bool ok;
    int64_t elems;
    int r[3], n[3], folded[3], L[3];
    bool on[3];
    int passes;
    size_t tab_off[3], clip_off, bytes;
};

static GwPlan gw_plan(int t, int c, int h, int w, double st, double sh, double sw) {
    GwPlan g = {};
    if (t < 1 || c < 1 || h < 1 || w < 1) return g;
    const int64_t planes = (int64_t)t * c, plane = (int64_t)h * w;  // (both halves bounded before their product is formed)
    if (planes > INT32_MAX || plane > INT32_MAX || planes * plane > INT32_MAX) return g;
    const int64_t elems = planes * plane;
    const double sig[3] = {st, sh, sw};
    const int ext[3] = {t, h, w};
    size_t off = 0;
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(sig[a]) || sig[a] < 0.0) return g;
        g.on[a] = sig[a] > 1e-15;
        g.L[a] = ext[a];
        if (!g.on[a]) continue;
        if (4.0 * sig[a] + 0.5 >= (double)GW_MAX_RADIUS + 1.0) return g;
        g.r[a] = (int)(4.0 * sig[a] + 0.5);
        g.folded[a] = 2 * (int64_t)g.r[a] + 1 > ext[a];
        g.n[a] = g.folded[a] ? ext[a] : 2 * g.r[a] + 1;
        g.tab_off[a] = off;
        off += ((size_t)g.n[a] * sizeof(double) + 255) / 256 * 256;
        ++g.passes;
    }
    g.elems = elems;
    g.clip_off = off;
    g.bytes = off + (g.passes >= 2 ? (size_t)elems * sizeof(float) : 0);
    g.ok = true;
    return g;
}

// Tile of a strided pass: preferred outputs along L, then whatever the LDS cap allows; *fits = false -> the global kernel.
static void gw_tile(int64_t L, int n, int cap, int pref, int least, int* R, int* S, int* whole, bool* fits) {
    *fits = true;
    *whole = 0;
    int64_t r = pref, s = r + n - 1;
    if (s >= L && L <= cap) {
        *whole = 1, *R = (int)L, *S = (int)L;
        return;
    }
    if (s > cap) {
        r = (int64_t)cap - (n - 1);
        s = cap;
        if (r < least) {
            if (L <= cap) {
                *whole = 1, *R = (int)L, *S = (int)L;
                return;
            }
            *fits = false;
            return;
        }
    }
    *R = (int)r, *S = (int)s;  // a window: s < L (either the preferred tile was shorter than the axis, or s = cap < L)
}

static int gw_launch(GwPass p, bool row_pass, hipStream_t stream) {
    if (row_pass) {  // R outputs and their halo per row (n <= 8193: at most 37 KiB), as many rows per workgroup as keep it near 40 KiB
        p.R = (int)(p.L < GW_ROW_TILE ? p.L : GW_ROW_TILE);
        p.S = p.R + p.n - 1;
        p.whole = 0;
        int rows = GW_ROW_LDS_FLOATS / p.S;
        rows = rows < 1 ? 1 : (rows > 16 ? 16 : rows);
        if (rows > p.outer) rows = (int)p.outer;
        p.ltiles = (p.L + p.R - 1) / p.R;
        p.ctiles = 1;
        p.tiles = p.ltiles * ((p.outer + rows - 1) / rows);
        const unsigned grid = (unsigned)(p.tiles < (1 << 20) ? p.tiles : (1 << 20));
        hipLaunchKernelGGL(gauss_wrap_row_kernel, dim3(grid), dim3(64 * rows), (size_t)rows * p.S * sizeof(float), stream, p);
        return check_launch("gauss_wrap_row_kernel");
    }
    bool fits;
    const int pref = p.n < 64 ? 64 : (p.n > 128 ? 128 : p.n);
    gw_tile(p.L, p.n, GW_ROWS_CAP, pref, 16, &p.R, &p.S, &p.whole, &fits);
    if (!fits) {
        hipLaunchKernelGGL(gauss_wrap_global_kernel, dim3(reduce_blocks(p.outer * p.L * p.inner, 256) * 8), dim3(256), 0, stream, p);
        return check_launch("gauss_wrap_global_kernel");
    }
    p.ltiles = (p.L + p.R - 1) / p.R;
    p.ctiles = (p.inner + GW_COLS - 1) / GW_COLS;
    p.tiles = p.ltiles * p.ctiles * p.outer;
    const size_t lds = (size_t)GW_COLS * p.S * sizeof(float);
    if (lds > 64 * 1024) {
        static unsigned long long served = 0;  // (once per device)
        const hipError_t rc = opt_in_dynamic_lds(reinterpret_cast<const void*>(gauss_wrap_strided_kernel), GW_LDS_FLOATS * 4, &served);
        if (rc != hipSuccess) {
            set_error("gauss_wrap: hipFuncSetAttribute: %s", hipGetErrorString(rc));
            return (int)rc;
        }
    }
    int groups = (p.R + GW_M - 1) / GW_M;
    groups = groups > 16 ? 16 : groups;
    const unsigned grid = (unsigned)(p.tiles < (1 << 20) ? p.tiles : (1 << 20));
    hipLaunchKernelGGL(gauss_wrap_strided_kernel, dim3(grid), dim3(64 * groups), lds, stream, p);
    return check_launch("gauss_wrap_strided_kernel");
}

}  // namespace maua

using namespace maua;

extern "C" {

int maua_gauss_wrap_supported(int t, int c, int h, int w, double sigma_t, double sigma_h, double sigma_w) {
    return gw_plan(t, c, h, w, sigma_t, sigma_h, sigma_w).ok ? 1 : 0;
}

size_t maua_gauss_wrap_workspace_bytes(int t, int c, int h, int w, double sigma_t, double sigma_h, double sigma_w) {
    const GwPlan g = gw_plan(t, c, h, w, sigma_t, sigma_h, sigma_w);
    return g.ok ? g.bytes : 0;
}

int maua_gauss_wrap(const float* x, float* y, int t, int c, int h, int w, double sigma_t, double sigma_h, double sigma_w, int roll_t,
                    void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(x && y, MAUA_E_INVAL, "gauss_wrap: null pointer");
    MAUA_REQUIRE(x != y, MAUA_E_INVAL, "gauss_wrap: x and y are the same buffer (the passes read their neighbours: not in place)");
    const GwPlan g = gw_plan(t, c, h, w, sigma_t, sigma_h, sigma_w);
    MAUA_REQUIRE(g.ok, MAUA_E_INVAL, "gauss_wrap: unsupported clip %d x %d x %d x %d with sigmas (%g, %g, %g): extents >= 1, at most 2^31 - 1 "
                 "elements, finite sigmas >= 0, radius int(4 sigma + 0.5) <= %d", t, c, h, w, sigma_t, sigma_h, sigma_w, GW_MAX_RADIUS);
    MAUA_REQUIRE(g.bytes == 0 || workspace, MAUA_E_INVAL, "gauss_wrap: null pointer (workspace of %zu bytes)", g.bytes);
    MAUA_REQUIRE(workspace_bytes >= g.bytes, MAUA_E_INVAL, "gauss_wrap: workspace too small (%zu bytes, needs %zu)", workspace_bytes, g.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int roll = (int)(((int64_t)roll_t % t + t) % t);
    const int64_t frame = (int64_t)c * h * w;
    if (g.passes == 0) {  // the rolled clip, bit for bit: frames roll .. T - 1, then frames 0 .. roll - 1
        hipError_t rc = hipMemcpyAsync(y, x + (int64_t)roll * frame, (size_t)(t - roll) * frame * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (rc == hipSuccess && roll)
            rc = hipMemcpyAsync(y + (int64_t)(t - roll) * frame, x, (size_t)roll * frame * sizeof(float), hipMemcpyDeviceToDevice, st);
        MAUA_REQUIRE(rc == hipSuccess, (int)rc, "gauss_wrap: hipMemcpyAsync: %s", hipGetErrorString(rc));
        return MAUA_OK;
    }
    char* ws = (char*)workspace;
    GwTables tabs = {};
    for (int a = 0; a < 3; ++a) {
        if (!g.on[a]) continue;
        tabs.a[a].sigma = a == 0 ? sigma_t : (a == 1 ? sigma_h : sigma_w);
        tabs.a[a].tab = (double*)(ws + g.tab_off[a]);
        tabs.a[a].r = g.r[a], tabs.a[a].n = g.n[a], tabs.a[a].L = g.L[a], tabs.a[a].folded = g.folded[a];
    }
    hipLaunchKernelGGL(gauss_wrap_weights_kernel, dim3(3), dim3(256), 0, st, tabs);
    int rc = check_launch("gauss_wrap_weights_kernel");
    if (rc) return rc;
    float* clip = g.passes >= 2 ? (float*)(ws + g.clip_off) : nullptr;
    const float* src = x;
    int left = g.passes;
    bool first = true;
    for (int a = 0; a < 3; ++a) {
        if (!g.on[a]) continue;
        GwPass p = {};
        p.src = src;
        p.dst = (left % 2 == 1) ? y : clip;  // the last pass (left == 1) writes y, the ones before it alternate
        p.tab = tabs.a[a].tab;
        p.n = g.n[a];
        p.L = g.L[a];
        p.T = t;
        p.per_frame = 1;
        const int off = g.folded[a] ? 0 : -g.r[a];
        if (a == 0) {
            p.outer = 1, p.inner = frame;
            p.shift = (int)((((int64_t)off + roll) % t + t) % t);
        } else {
            p.outer = a == 1 ? (int64_t)t * c : (int64_t)t * c * h;
            p.inner = a == 1 ? w : 1;
            p.per_frame = a == 1 ? c : (int64_t)c * h;
            p.shift = (int)(((int64_t)off % p.L + p.L) % p.L);
            p.roll = first ? roll : 0;
        }
        rc = gw_launch(p, a == 2, st);
        if (rc) return rc;
        src = p.dst;
        first = false;
        --left;
    }
    return MAUA_OK;
}

}  // extern "C"
