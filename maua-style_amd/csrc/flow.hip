// Optical flow for vid_img's temporal path (the reference estimates it with downloaded networks, flow.py:32-74 / load.py:141-188):
// a weight-free coarse-to-fine TV-L1 solver (Zach, Pock, Bischof 2007, duality scheme; Wedel et al. 2009 warping + median filter;
// the per-pixel scheme as written down by Sanchez, Meinhardt-Llopis, Facciolo, IPOL 2013) and the reference's occlusion / reliability
// mask (flow.py:77-137) restated on the device.  DESIGN.md section "Optical flow" has the exact algorithm.
//
// All planes are fp32, row-major H x W, one plane per component.  Solver state = 6 planes [u1][u2][p11][p12][p21][p22] (u = flow,
// p = dual of each component's forward gradient); per-warp fields = 3 planes [I1wx][I1wy][rho_c].
// Every TV-L1 iteration goes through tv_u / tv_p below, in both kernel forms, with contraction off: the temporally blocked kernel
// (K iterations per launch, state in LDS) is bit-identical to K launches of the single-step kernel.  No float atomics anywhere.
// hipcc-flags: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
#include "common.hpp"

#pragma clang fp contract(off)

namespace maua {

namespace {

constexpr float TV_THETA = 0.3f;
constexpr float TV_LT = 0.15f * 0.3f;    // lambda * theta
constexpr float TV_TAUT = 0.25f / 0.3f;  // tau / theta
constexpr int PX = 16;                    // per-pixel kernels: 16 x 16 workgroups
constexpr int BT = 32;                    // blocked TV-L1: 32 x 32 interior per workgroup
constexpr int BT_THREADS = 512;
constexpr int BT_KMAX = 16;               // (32 + 2 K)^2 positions x 9 floats <= 160 KiB of LDS
constexpr int ER = 20;                    // erosion radius: scipy gaussian_filter(sigma 5, truncate 4)

bool dims_ok(int h, int w) { return h > 0 && w > 0 && h <= (1 << 16) && w <= (1 << 16) && (int64_t)h * w <= (1ll << 28); }

// ---- the shared TV-L1 update -------------------------------------------------------------------------------------------
// u step: thresholding of rho = rho_c + grad(I1w) . u, then u = v + theta div p.  d1 / d2 = div p1 / div p2.
__device__ __forceinline__ void tv_u(float u1, float u2, float wx, float wy, float rc, float d1, float d2, float& o1, float& o2) {
    const float g2 = wx * wx + wy * wy;
    const float rho = rc + (wx * u1 + wy * u2);
    float v1, v2;
    if (rho < -TV_LT * g2) {
        v1 = u1 + TV_LT * wx;
        v2 = u2 + TV_LT * wy;
    } else if (rho > TV_LT * g2) {
        v1 = u1 - TV_LT * wx;
        v2 = u2 - TV_LT * wy;
    } else if (g2 < 1e-10f) {
        v1 = u1;
        v2 = u2;
    } else {
        const float f = -rho / g2;
        v1 = u1 + f * wx;
        v2 = u2 + f * wy;
    }
    o1 = v1 + TV_THETA * d1;
    o2 = v2 + TV_THETA * d2;
}

// div p = (p_x(x) - p_x(x - 1)) + (p_y(y) - p_y(y - 1)): callers pass 0 for p_x at x = W-1 / x - 1 < 0 and p_y at y = H-1 / y - 1 < 0
// (the negative adjoint of the forward difference that is zero on the last column / row)
__device__ __forceinline__ float tv_div(float xh, float xl, float yh, float yl) { return (xh - xl) + (yh - yl); }

// p step of one component: p = (p + taut grad u) / (1 + taut |grad u|)
__device__ __forceinline__ void tv_p(float pa, float pb, float gx, float gy, float& oa, float& ob) {
    const float ng = 1.0f + TV_TAUT * sqrtf(gx * gx + gy * gy);
    oa = (pa + TV_TAUT * gx) / ng;
    ob = (pb + TV_TAUT * gy) / ng;
}

// ---- images ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grey_kernel(const uint8_t* __restrict__ rgb, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    out[i] = (0.299f * r + 0.587f * g) + 0.114f * b;
}

struct PyrWeights {
    float w[8];
};

// Gaussian (sigma 0.6 sqrt(1/eta^2 - 1), eta 0.5) sampled at the half-pixel centre 2o + 0.5 of the output pixel: 8 taps at input
// 2o - 3 .. 2o + 4, edge pixels replicated; output side = ceil(side / 2).  Rows first into an LDS tile, then columns.
__global__ void __launch_bounds__(256) pyr_down_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w, int oh,
                                                       int ow, PyrWeights pw) {
    __shared__ float rows[2 * PX + 6][PX + 1];
    const int tx = threadIdx.x & (PX - 1), ty = threadIdx.x >> 4;
    const int ox0 = blockIdx.x * PX, oy0 = blockIdx.y * PX;
    const int ox = ox0 + tx;
    const int cx = min(ox, ow - 1);
    for (int r = ty; r < 2 * PX + 6; r += PX) {
        const int iy = min(max(2 * oy0 - 3 + r, 0), h - 1);
        const float* row = in + (int64_t)iy * w;
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) s = s + pw.w[t] * row[min(max(2 * cx - 3 + t, 0), w - 1)];
        rows[r][tx] = s;
    }
    __syncthreads();
    const int oy = oy0 + ty;
    if (ox >= ow || oy >= oh) return;
    float s = 0.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) s = s + pw.w[t] * rows[2 * ty + t][tx];
    out[(int64_t)oy * ow + ox] = s;
}

// centred difference with clamped neighbours
__device__ __forceinline__ void grad_at(const float* __restrict__ I, int h, int w, int x, int y, float& gx, float& gy) {
    const int64_t r = (int64_t)y * w;
    gx = 0.5f * (I[r + min(x + 1, w - 1)] - I[r + max(x - 1, 0)]);
    gy = 0.5f * (I[(int64_t)min(y + 1, h - 1) * w + x] - I[(int64_t)max(y - 1, 0) * w + x]);
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float fx, float fy) {
    return (1.0f - fy) * ((1.0f - fx) * a + fx * b) + fy * ((1.0f - fx) * c + fx * d);
}

// I1 and its gradient sampled bilinearly at x + u (coordinates clamped to the frame); fields = [I1wx][I1wy][rho_c]
__global__ void __launch_bounds__(256) warp_prep_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                        const float* __restrict__ u, float* __restrict__ fld, int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const int64_t hw = (int64_t)h * w, i = (int64_t)y * w + x;
    const float u1 = u[i], u2 = u[hw + i];
    const float X = fminf(fmaxf((float)x + u1, 0.0f), (float)(w - 1));
    const float Y = fminf(fmaxf((float)y + u2, 0.0f), (float)(h - 1));
    const int x0 = min((int)floorf(X), max(w - 2, 0)), y0 = min((int)floorf(Y), max(h - 2, 0));
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float fx = X - (float)x0, fy = Y - (float)y0;
    float gx[4], gy[4];
    grad_at(i1, h, w, x0, y0, gx[0], gy[0]);
    grad_at(i1, h, w, x1, y0, gx[1], gy[1]);
    grad_at(i1, h, w, x0, y1, gx[2], gy[2]);
    grad_at(i1, h, w, x1, y1, gx[3], gy[3]);
    const float iw = lerp2(i1[(int64_t)y0 * w + x0], i1[(int64_t)y0 * w + x1], i1[(int64_t)y1 * w + x0], i1[(int64_t)y1 * w + x1], fx, fy);
    const float wx = lerp2(gx[0], gx[1], gx[2], gx[3], fx, fy);
    const float wy = lerp2(gy[0], gy[1], gy[2], gy[3], fx, fy);
    fld[i] = wx;
    fld[hw + i] = wy;
    fld[2 * hw + i] = ((iw - wx * u1) - wy * u2) - i0[i];
}

// ---- TV-L1 iteration, single step (halo 1, state double-buffered) -----------------------------------------------------------
// u after this iteration at (x, y), from the state before it
__device__ __forceinline__ void u_at(const float* __restrict__ fld, const float* __restrict__ s, int64_t hw, int h, int w, int x, int y,
                                     float& o1, float& o2) {
    const int64_t i = (int64_t)y * w + x;
    const float d1 = tv_div(x < w - 1 ? s[2 * hw + i] : 0.0f, x > 0 ? s[2 * hw + i - 1] : 0.0f, y < h - 1 ? s[3 * hw + i] : 0.0f,
                            y > 0 ? s[3 * hw + i - w] : 0.0f);
    const float d2 = tv_div(x < w - 1 ? s[4 * hw + i] : 0.0f, x > 0 ? s[4 * hw + i - 1] : 0.0f, y < h - 1 ? s[5 * hw + i] : 0.0f,
                            y > 0 ? s[5 * hw + i - w] : 0.0f);
    tv_u(s[i], s[hw + i], fld[i], fld[hw + i], fld[2 * hw + i], d1, d2, o1, o2);
}

__global__ void __launch_bounds__(256) tvl1_step_kernel(const float* __restrict__ fld, const float* __restrict__ s, float* __restrict__ o,
                                                        int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const int64_t hw = (int64_t)h * w, i = (int64_t)y * w + x;
    float a1, a2, r1 = 0.0f, r2 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    u_at(fld, s, hw, h, w, x, y, a1, a2);
    if (x < w - 1) u_at(fld, s, hw, h, w, x + 1, y, r1, r2);
    if (y < h - 1) u_at(fld, s, hw, h, w, x, y + 1, d1, d2);
    const float g1x = x < w - 1 ? r1 - a1 : 0.0f, g1y = y < h - 1 ? d1 - a1 : 0.0f;
    const float g2x = x < w - 1 ? r2 - a2 : 0.0f, g2y = y < h - 1 ? d2 - a2 : 0.0f;
    float q11, q12, q21, q22;
    tv_p(s[2 * hw + i], s[3 * hw + i], g1x, g1y, q11, q12);
    tv_p(s[4 * hw + i], s[5 * hw + i], g2x, g2y, q21, q22);
    o[i] = a1;
    o[hw + i] = a2;
    o[2 * hw + i] = q11;
    o[3 * hw + i] = q12;
    o[4 * hw + i] = q21;
    o[5 * hw + i] = q22;
}

// ---- TV-L1 iterations, temporally blocked --------------------------------------------------------------------------------------
// One workgroup: a 32 x 32 interior plus a halo of k; the 6 state planes and the 3 fields of the (32 + 2k)^2 positions live in LDS.
// Iteration s (0-based) updates u on positions [s + 1, L - s) and p on [s + 1, L - s - 1) of each axis (L = 32 + 2k): after k
// iterations the interior [k, k + 32) is exact.  Positions outside the frame are never read by positions inside it (the boundary
// rules select 0 there), so they are skipped.
__global__ void __launch_bounds__(BT_THREADS) tvl1_blocked_kernel(const float* __restrict__ fld, const float* __restrict__ s,
                                                                  float* __restrict__ o, int h, int w, int k) {
    extern __shared__ float lds[];
    const int L = BT + 2 * k, LL = L * L;
    float* su1 = lds;
    float* su2 = su1 + LL;
    float* sp11 = su2 + LL;
    float* sp12 = sp11 + LL;
    float* sp21 = sp12 + LL;
    float* sp22 = sp21 + LL;
    float* swx = sp22 + LL;
    float* swy = swx + LL;
    float* src = swy + LL;
    const int gx0 = blockIdx.x * BT - k, gy0 = blockIdx.y * BT - k;
    const int64_t hw = (int64_t)h * w;
    for (int q = threadIdx.x; q < LL; q += BT_THREADS) {
        const int j = q / L, i = q - j * L, x = gx0 + i, y = gy0 + j;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const int64_t g = (int64_t)y * w + x;
            su1[q] = s[g];
            su2[q] = s[hw + g];
            sp11[q] = s[2 * hw + g];
            sp12[q] = s[3 * hw + g];
            sp21[q] = s[4 * hw + g];
            sp22[q] = s[5 * hw + g];
            swx[q] = fld[g];
            swy[q] = fld[hw + g];
            src[q] = fld[2 * hw + g];
        }
    }
    __syncthreads();
    for (int st = 0; st < k; ++st) {
        const int lo = st + 1, hu = L - st, hp = L - st - 1;
        const int nu = hu - lo;
        for (int q = threadIdx.x; q < nu * nu; q += BT_THREADS) {
            const int j = lo + q / nu, i = lo + q % nu, x = gx0 + i, y = gy0 + j;
            if (x < 0 || x >= w || y < 0 || y >= h) continue;
            const int p = j * L + i;
            const float d1 = tv_div(x < w - 1 ? sp11[p] : 0.0f, x > 0 ? sp11[p - 1] : 0.0f, y < h - 1 ? sp12[p] : 0.0f,
                                    y > 0 ? sp12[p - L] : 0.0f);
            const float d2 = tv_div(x < w - 1 ? sp21[p] : 0.0f, x > 0 ? sp21[p - 1] : 0.0f, y < h - 1 ? sp22[p] : 0.0f,
                                    y > 0 ? sp22[p - L] : 0.0f);
            float a1, a2;
            tv_u(su1[p], su2[p], swx[p], swy[p], src[p], d1, d2, a1, a2);
            su1[p] = a1;  // (own position only: p of the neighbours is read, never u)
            su2[p] = a2;
        }
        __syncthreads();
        const int np = hp - lo;
        for (int q = threadIdx.x; q < np * np; q += BT_THREADS) {
            const int j = lo + q / np, i = lo + q % np, x = gx0 + i, y = gy0 + j;
            if (x < 0 || x >= w || y < 0 || y >= h) continue;
            const int p = j * L + i;
            const float a1 = su1[p], a2 = su2[p];
            const float g1x = x < w - 1 ? su1[p + 1] - a1 : 0.0f, g1y = y < h - 1 ? su1[p + L] - a1 : 0.0f;
            const float g2x = x < w - 1 ? su2[p + 1] - a2 : 0.0f, g2y = y < h - 1 ? su2[p + L] - a2 : 0.0f;
            float q11, q12, q21, q22;
            tv_p(sp11[p], sp12[p], g1x, g1y, q11, q12);
            tv_p(sp21[p], sp22[p], g2x, g2y, q21, q22);
            sp11[p] = q11;
            sp12[p] = q12;
            sp21[p] = q21;
            sp22[p] = q22;
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < BT * BT; q += BT_THREADS) {
        const int j = k + q / BT, i = k + q % BT, x = gx0 + i, y = gy0 + j;
        if (x >= w || y >= h) continue;
        const int p = j * L + i;
        const int64_t g = (int64_t)y * w + x;
        o[g] = su1[p];
        o[hw + g] = su2[p];
        o[2 * hw + g] = sp11[p];
        o[3 * hw + g] = sp12[p];
        o[4 * hw + g] = sp21[p];
        o[5 * hw + g] = sp22[p];
    }
}

// ---- 5 x 5 median (edge pixels replicated), exact: the element of rank 12 (ties broken by window position) -------------------
__global__ void __launch_bounds__(256) median5_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    const int64_t plane = (int64_t)blockIdx.z * h * w;
    if (x >= w || y >= h) return;
    float v[25];
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float* row = in + plane + (int64_t)min(max(y + dy - 2, 0), h - 1) * w;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) v[dy * 5 + dx] = row[min(max(x + dx - 2, 0), w - 1)];
    }
    float med = v[0];
#pragma unroll
    for (int a = 0; a < 25; ++a) {
        int rank = 0;
#pragma unroll
        for (int b = 0; b < 25; ++b) rank += (v[b] < v[a]) || (b < a && v[b] == v[a]);
        med = rank == 12 ? v[a] : med;
    }
    out[plane + (int64_t)y * w + x] = med;
}

// ---- bilinear upsampling, half-pixel centres (F.interpolate(align_corners=False)), values times `scale` ------------------------
__global__ void __launch_bounds__(256) upsample_kernel(const float* __restrict__ in, int ch, int cw, float* __restrict__ out, int h, int w,
                                                       float ry, float rx, float scale) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const float* src = in + (int64_t)blockIdx.z * ch * cw;
    const float sx = fmaxf(((float)x + 0.5f) * rx - 0.5f, 0.0f), sy = fmaxf(((float)y + 0.5f) * ry - 0.5f, 0.0f);
    const int x0 = min((int)sx, cw - 1), y0 = min((int)sy, ch - 1);
    const int x1 = min(x0 + 1, cw - 1), y1 = min(y0 + 1, ch - 1);
    const float fx = sx - (float)x0, fy = sy - (float)y0;
    const float v = lerp2(src[(int64_t)y0 * cw + x0], src[(int64_t)y0 * cw + x1], src[(int64_t)y1 * cw + x0], src[(int64_t)y1 * cw + x1],
                          fx, fy);
    out[(int64_t)blockIdx.z * h * w + (int64_t)y * w + x] = v * scale;
}

// ---- reliability mask: reference flow.py:77-137 (check_consistency) ----------------------------------------------------------------
// Types and operation order as numpy evaluates the reference: coordinates int64 + fp32 flow -> fp64; the bilinear look-up of flow2,
// the round-trip distance and its threshold in fp64 (flow1 ** 2 squared in fp32 first); the motion edge in fp64 (np.diff with
// append=0 promotes to fp64) against a threshold computed in fp32.  Classes: 1 reliable, -1 round trip inconsistent, 0 outside
// the frame / motion edge.  (flipped channels: component 0 = v, 1 = u.)
__global__ void __launch_bounds__(256) consistency_kernel(const float* __restrict__ f1, const float* __restrict__ f2, int8_t* __restrict__ cls,
                                                          int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const int64_t hw = (int64_t)h * w, i = (int64_t)y * w + x;
    const float fv = f1[hw + i], fu = f1[i];
    const double wy = (double)y + (double)fv, wx = (double)x + (double)fu;
    const double cy = fmin(fmax(wy, 0.0), (double)(h - 2)), cx = fmin(fmax(wx, 0.0), (double)(w - 2));
    const double fy = floor(cy), fx = floor(cx);
    const int iy = (int)fy, ix = (int)fx;
    const double a0 = cy - fy, a1 = cx - fx;
    const int64_t i00 = (int64_t)iy * w + ix, i01 = i00 + 1, i10 = i00 + w, i11 = i10 + 1;
    double wc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* g = f2 + (c == 0 ? hw : 0);  // flipped: channel 0 = v
        const double b0 = (1.0 - a1) * (double)g[i00] + a1 * (double)g[i01];
        const double b1 = (1.0 - a1) * (double)g[i10] + a1 * (double)g[i11];
        wc[c] = (1.0 - a0) * b0 + a0 * b1;
    }
    const double dy = (wy + wc[0]) - (double)y, dx = (wx + wc[1]) - (double)x;
    const double sq = dy * dy + dx * dx;
    const double thr = 0.01 * ((wc[0] * wc[0] + (double)(fv * fv)) + (wc[1] * wc[1] + (double)(fu * fu))) + 0.5;
    int r = sq >= thr ? -1 : 1;
    if (wy < 0.0 || wx < 0.0 || wy >= (double)(h - 1) || wx >= (double)(w - 1)) r = 0;
    double me = 0.0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* g = f1 + (c == 0 ? hw : 0);
        const double here = (double)g[i];
        const double ddx = (x < w - 1 ? (double)g[i + 1] : 0.0) - here;
        const double ddy = (y < h - 1 ? (double)g[i + w] : 0.0) - here;
        me = c == 0 ? ddx * ddx + ddy * ddy : me + (ddx * ddx + ddy * ddy);
    }
    const float mt = 0.01f * (fv * fv + fu * fu) + 0.002f;
    if (me > (double)mt && r != -1) r = 0;
    cls[i] = (int8_t)r;
}

// scipy.ndimage.gaussian_filter(int64 field, sigma 5) truncates to the integer dtype after each 1-D pass (axis 0, then axis 1); for a
// field in {-1, 0, 1} the result clipped to [0, 1] is 1 exactly where the whole 41 x 41 window (clamped to the frame) is 1: an erosion.
// Pass 1 (columns): 1 where the column window is all 1.  Pass 2 (rows): the PNG byte (1 - r) * 255.
__global__ void __launch_bounds__(256) erode_cols_kernel(const int8_t* __restrict__ cls, uint8_t* __restrict__ t, int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    int all = 1;
    for (int yy = max(y - ER, 0); yy <= min(y + ER, h - 1); ++yy) all &= cls[(int64_t)yy * w + x] == 1;
    t[(int64_t)y * w + x] = (uint8_t)all;
}

__global__ void __launch_bounds__(256) erode_rows_kernel(const uint8_t* __restrict__ t, uint8_t* __restrict__ out, int h, int w) {
    const int x = blockIdx.x * PX + (threadIdx.x & (PX - 1)), y = blockIdx.y * PX + (threadIdx.x >> 4);
    if (x >= w || y >= h) return;
    const uint8_t* row = t + (int64_t)y * w;
    int all = 1;
    for (int xx = max(x - ER, 0); xx <= min(x + ER, w - 1); ++xx) all &= row[xx];
    out[(int64_t)y * w + x] = all ? 0 : 255;
}

dim3 px_grid(int h, int w, int planes = 1) { return dim3((w + PX - 1) / PX, (h + PX - 1) / PX, planes); }

PyrWeights pyr_weights() {
    const double sigma = 0.6 * sqrt(1.0 / (0.5 * 0.5) - 1.0);
    double g[8], s = 0.0;
    for (int t = 0; t < 8; ++t) {
        const double d = t - 3.5;
        g[t] = exp(-d * d / (2.0 * sigma * sigma));
        s += g[t];
    }
    PyrWeights pw;
    for (int t = 0; t < 8; ++t) pw.w[t] = (float)(g[t] / s);
    return pw;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int launch_blocked(const float* fld, const float* s, float* o, int h, int w, int k, hipStream_t st) {
    static unsigned long long served = 0;  // (once per device)
    const int L = BT + 2 * BT_KMAX;
    if (opt_in_dynamic_lds(reinterpret_cast<const void*>(tvl1_blocked_kernel), L * L * 9 * 4, &served) != hipSuccess)
        return check_launch("flow_tvl1_blocked (LDS opt-in)");
    const size_t lds = (size_t)(BT + 2 * k) * (BT + 2 * k) * 9 * sizeof(float);
    tvl1_blocked_kernel<<<dim3((w + BT - 1) / BT, (h + BT - 1) / BT), BT_THREADS, lds, st>>>(fld, s, o, h, w, k);
    return check_launch("flow_tvl1_blocked");
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_flow_levels(int h, int w, int max_levels) {
    if (!dims_ok(h, w) || max_levels < 1) return 0;
    int n = 1;
    while (n < max_levels && ((h + 1) / 2) >= 16 && ((w + 1) / 2) >= 16) {
        h = (h + 1) / 2;
        w = (w + 1) / 2;
        ++n;
    }
    return n;
}

extern "C" int maua_flow_grey_u8(const uint8_t* rgb, float* out, int h, int w, maua_stream_t stream) {
    MAUA_REQUIRE(rgb && out, MAUA_E_INVAL, "flow_grey_u8: null pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_grey_u8: bad size %dx%d", h, w);
    const int64_t n = (int64_t)h * w;
    grey_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(rgb, out, n);
    return check_launch("flow_grey_u8");
}

extern "C" int maua_flow_pyr_down(const float* in, float* out, int h, int w, maua_stream_t stream) {
    MAUA_REQUIRE(in && out, MAUA_E_INVAL, "flow_pyr_down: null pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_pyr_down: bad size %dx%d", h, w);
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    pyr_down_kernel<<<px_grid(oh, ow), 256, 0, (hipStream_t)stream>>>(in, out, h, w, oh, ow, pyr_weights());
    return check_launch("flow_pyr_down");
}

extern "C" int maua_flow_warp_prep(const float* i0, const float* i1, const float* u, float* fields, int h, int w, maua_stream_t stream) {
    MAUA_REQUIRE(i0 && i1 && u && fields, MAUA_E_INVAL, "flow_warp_prep: null pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_warp_prep: bad size %dx%d", h, w);
    warp_prep_kernel<<<px_grid(h, w), 256, 0, (hipStream_t)stream>>>(i0, i1, u, fields, h, w);
    return check_launch("flow_warp_prep");
}

extern "C" int maua_flow_tvl1_step(const float* fields, const float* state_in, float* state_out, int h, int w, maua_stream_t stream) {
    MAUA_REQUIRE(fields && state_in && state_out && state_in != state_out, MAUA_E_INVAL, "flow_tvl1_step: null or aliased pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_tvl1_step: bad size %dx%d", h, w);
    tvl1_step_kernel<<<px_grid(h, w), 256, 0, (hipStream_t)stream>>>(fields, state_in, state_out, h, w);
    return check_launch("flow_tvl1_step");
}

extern "C" int maua_flow_tvl1_blocked(const float* fields, const float* state_in, float* state_out, int h, int w, int k,
                                      maua_stream_t stream) {
    MAUA_REQUIRE(fields && state_in && state_out && state_in != state_out, MAUA_E_INVAL, "flow_tvl1_blocked: null or aliased pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_tvl1_blocked: bad size %dx%d", h, w);
    MAUA_REQUIRE(k >= 1 && k <= BT_KMAX, MAUA_E_INVAL, "flow_tvl1_blocked: k = %d outside 1..%d", k, BT_KMAX);
    return launch_blocked(fields, state_in, state_out, h, w, k, (hipStream_t)stream);
}

extern "C" int maua_flow_median5(const float* in, float* out, int h, int w, int planes, maua_stream_t stream) {
    MAUA_REQUIRE(in && out && in != out, MAUA_E_INVAL, "flow_median5: null or aliased pointer");
    MAUA_REQUIRE(dims_ok(h, w) && planes >= 1 && planes <= 64, MAUA_E_INVAL, "flow_median5: bad size");
    median5_kernel<<<px_grid(h, w, planes), 256, 0, (hipStream_t)stream>>>(in, out, h, w);
    return check_launch("flow_median5");
}

extern "C" int maua_flow_upsample(const float* in, int ch, int cw, float* out, int h, int w, int planes, float scale, maua_stream_t stream) {
    MAUA_REQUIRE(in && out, MAUA_E_INVAL, "flow_upsample: null pointer");
    MAUA_REQUIRE(dims_ok(h, w) && dims_ok(ch, cw) && planes >= 1 && planes <= 64, MAUA_E_INVAL, "flow_upsample: bad size");
    upsample_kernel<<<px_grid(h, w, planes), 256, 0, (hipStream_t)stream>>>(in, ch, cw, out, h, w, (float)ch / (float)h,
                                                                            (float)cw / (float)w, scale);
    return check_launch("flow_upsample");
}

extern "C" size_t maua_flow_consistency_workspace_bytes(int h, int w) {
    if (!dims_ok(h, w)) return 0;
    return 2 * align256((size_t)h * w);
}

extern "C" int maua_flow_consistency(const float* flow1, const float* flow2, uint8_t* out, int h, int w, void* workspace,
                                     size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(flow1 && flow2 && out && workspace, MAUA_E_INVAL, "flow_consistency: null pointer");
    MAUA_REQUIRE(dims_ok(h, w) && h >= 2 && w >= 2, MAUA_E_INVAL, "flow_consistency: bad size %dx%d (both sides >= 2)", h, w);
    MAUA_REQUIRE(workspace_bytes >= maua_flow_consistency_workspace_bytes(h, w), MAUA_E_WORKSPACE, "flow_consistency: workspace too small");
    int8_t* cls = static_cast<int8_t*>(workspace);
    uint8_t* t = static_cast<uint8_t*>(workspace) + align256((size_t)h * w);
    const hipStream_t st = (hipStream_t)stream;
    consistency_kernel<<<px_grid(h, w), 256, 0, st>>>(flow1, flow2, cls, h, w);
    erode_cols_kernel<<<px_grid(h, w), 256, 0, st>>>(cls, t, h, w);
    erode_rows_kernel<<<px_grid(h, w), 256, 0, st>>>(t, out, h, w);
    return check_launch("flow_consistency");
}

// Workspace of maua_flow_tvl1: grey pyramids of both frames, two solver states and the fields at the finest size, a 2-plane scratch.
extern "C" size_t maua_flow_tvl1_workspace_bytes(int h, int w, int levels) {
    if (!dims_ok(h, w) || levels < 1 || levels > 8 || levels > maua_flow_levels(h, w, levels)) return 0;
    const size_t hw = (size_t)h * w;
    size_t b = 0;
    for (int l = 0, lh = h, lw = w; l < levels; ++l, lh = (lh + 1) / 2, lw = (lw + 1) / 2) b += 2 * align256((size_t)lh * lw * 4);
    return b + 2 * align256(6 * hw * 4) + align256(3 * hw * 4) + align256(2 * hw * 4);
}

extern "C" int maua_flow_tvl1(const uint8_t* rgb1, const uint8_t* rgb2, float* flow, int h, int w, int levels, int warps, int iters,
                              int block_k, void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(rgb1 && rgb2 && flow && workspace, MAUA_E_INVAL, "flow_tvl1: null pointer");
    MAUA_REQUIRE(dims_ok(h, w), MAUA_E_INVAL, "flow_tvl1: bad size %dx%d", h, w);
    MAUA_REQUIRE(levels >= 1 && levels <= 8 && levels <= maua_flow_levels(h, w, levels), MAUA_E_INVAL, "flow_tvl1: %d levels for %dx%d", levels, h, w);
    MAUA_REQUIRE(warps >= 1 && warps <= 100 && iters >= 1 && iters <= 100000 && block_k >= 0 && block_k <= BT_KMAX, MAUA_E_INVAL,
                 "flow_tvl1: warps %d / iterations %d / block_k %d", warps, iters, block_k);
    MAUA_REQUIRE(workspace_bytes >= maua_flow_tvl1_workspace_bytes(h, w, levels), MAUA_E_WORKSPACE, "flow_tvl1: workspace too small");
    const hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(workspace);
    int lh[8], lw[8];
    float *I0[8], *I1[8];
    for (int l = 0; l < levels; ++l) {
        lh[l] = l ? (lh[l - 1] + 1) / 2 : h;
        lw[l] = l ? (lw[l - 1] + 1) / 2 : w;
        const size_t b = align256((size_t)lh[l] * lw[l] * 4);
        I0[l] = reinterpret_cast<float*>(base);
        I1[l] = reinterpret_cast<float*>(base + b);
        base += 2 * b;
    }
    const size_t hw = (size_t)h * w;
    float* A = reinterpret_cast<float*>(base);
    float* B = reinterpret_cast<float*>(base + align256(6 * hw * 4));
    float* F = reinterpret_cast<float*>(base + 2 * align256(6 * hw * 4));
    float* T = reinterpret_cast<float*>(base + 2 * align256(6 * hw * 4) + align256(3 * hw * 4));
    int rc;
    if ((rc = maua_flow_grey_u8(rgb1, I0[0], h, w, stream)) != 0) return rc;
    if ((rc = maua_flow_grey_u8(rgb2, I1[0], h, w, stream)) != 0) return rc;
    for (int l = 1; l < levels; ++l) {
        if ((rc = maua_flow_pyr_down(I0[l - 1], I0[l], lh[l - 1], lw[l - 1], stream)) != 0) return rc;
        if ((rc = maua_flow_pyr_down(I1[l - 1], I1[l], lh[l - 1], lw[l - 1], stream)) != 0) return rc;
    }
    for (int l = levels - 1; l >= 0; --l) {
        const int H = lh[l], W = lw[l];
        const size_t n = (size_t)H * W;
        // state at this level: u from the coarser level (x 1/eta) or zero, p zero
        if (l == levels - 1) {
            MAUA_REQUIRE(hipMemsetAsync(A, 0, 6 * n * 4, st) == hipSuccess, (int)hipErrorLaunchFailure, "flow_tvl1: memset failed");
        } else {
            if ((rc = maua_flow_upsample(A, lh[l + 1], lw[l + 1], B, H, W, 2, 2.0f, stream)) != 0) return rc;
            MAUA_REQUIRE(hipMemsetAsync(B + 2 * n, 0, 4 * n * 4, st) == hipSuccess, (int)hipErrorLaunchFailure, "flow_tvl1: memset failed");
            float* t = A;
            A = B;
            B = t;
        }
        for (int wp = 0; wp < warps; ++wp) {
            if ((rc = maua_flow_warp_prep(I0[l], I1[l], A, F, H, W, stream)) != 0) return rc;
            for (int it = 0; it < iters;) {
                const int k = block_k >= 2 ? (iters - it < block_k ? iters - it : block_k) : 1;
                rc = block_k >= 2 ? launch_blocked(F, A, B, H, W, k, st) : maua_flow_tvl1_step(F, A, B, H, W, stream);
                if (rc != 0) return rc;
                float* t = A;
                A = B;
                B = t;
                it += k;
            }
            if ((rc = maua_flow_median5(A, T, H, W, 2, stream)) != 0) return rc;
            MAUA_REQUIRE(hipMemcpyAsync(A, T, 2 * n * 4, hipMemcpyDeviceToDevice, st) == hipSuccess, (int)hipErrorLaunchFailure,
                         "flow_tvl1: copy failed");
        }
    }
    MAUA_REQUIRE(hipMemcpyAsync(flow, A, 2 * hw * 4, hipMemcpyDeviceToDevice, st) == hipSuccess, (int)hipErrorLaunchFailure,
                 "flow_tvl1: copy failed");
    return MAUA_OK;
}
