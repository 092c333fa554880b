// The temporally consistent vid_img loop's image-space steps (style._vid_img_flow with the plan field temporal_device = 1), kept on the
// device so that the previous frame, the warp grid and the reliability mask never leave HBM between two optimize calls:
//   * load.flow_warp_map (reference load.py:191-214): flow in pixels -> fractions of the image size, scipy's gaussian_filter (sigma 5,
//     41 taps, `reflect` boundary, rows then columns, fp64 sums, fp32 intermediate), + the identity grid on [-1, 1]^2, bilinear resize;
//   * F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False) (reference style.py:253,281), with the
//     temporal blend of style.py:286 as an optional second output of the same pass over the previous frame;
//   * load.reliable_flow_weighting + F.interpolate (reference load.py:217-218, style.py:282): mask bytes -> [0, 1] floats, resized.
// All HBM-bound stencils and gathers over a few planes: no matrix cores.  No kernel here may hold packed fp32 instructions (they run
// between two optimize calls, possibly beside another stream's MFMA kernels; tests/test_abi.py keeps the list of kernels that do closed):
// hipcc-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
#include <math.h>

#include "common.hpp"

namespace maua {

constexpr int WG_RADIUS = 20;  // int(4 * 5 + 0.5): scipy's truncate = 4 at sigma 5
constexpr int WG_TILE = 32;    // output tile (rows and columns) of one workgroup
constexpr int WG_IN = WG_TILE + 2 * WG_RADIUS;

struct GaussTaps {
    double w[WG_RADIUS + 1];  // w[k] = weight at distance k from the centre (symmetric), normalised by the sum of all 41
};

// scipy's `reflect` extension (d c b a | a b c d | d c b a), repeated as often as the side is shorter than the reach
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - 1 - m;
}

// One component (blockIdx.z: 0 = u / w, 1 = v / h) of one 32 x 32 tile: the tile and its halo go to LDS once (72 x 72 values, reflected
// at the borders), the row-axis pass (axis 0: 41 rows per output) and the column-axis pass (axis 1) both read LDS with the lanes along
// a row, so no thread walks strided rows of global memory and the 32 lanes the LDS serves together read 32 neighbouring banks.  Sums in fp64 in scipy's order for symmetric
// filters (centre, then pairs from the outside in); the intermediate is rounded to fp32 as scipy's float32 output array does.
// out[z][y][x] = float(double(filtered) + linspace(-1, 1, side)[index]) - the fp64 sum numpy forms before its astype(float32).
__global__ void __launch_bounds__(256) flow_warp_smooth_kernel(const float* __restrict__ flo, float* __restrict__ out, int h, int w,
                                                               GaussTaps taps) {
    __shared__ float tile[WG_IN][WG_IN];
    __shared__ float mid[WG_TILE][WG_IN];
    const int z = blockIdx.z;
    const int x0 = blockIdx.x * WG_TILE, y0 = blockIdx.y * WG_TILE;
    const float side = z == 0 ? (float)w : (float)h;
    for (int e = threadIdx.x; e < WG_IN * WG_IN; e += 256) {
        const int r = e / WG_IN, c = e - r * WG_IN;
        const int gy = reflect_index(y0 - WG_RADIUS + r, h), gx = reflect_index(x0 - WG_RADIUS + c, w);
        tile[r][c] = __fdiv_rn(flo[((int64_t)gy * w + gx) * 2 + z], side);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < WG_TILE * WG_IN; e += 256) {  // axis 0
        const int r = e / WG_IN, c = e - r * WG_IN;
        double acc = (double)tile[r + WG_RADIUS][c] * taps.w[0];
#pragma unroll
        for (int k = WG_RADIUS; k >= 1; --k) acc += ((double)tile[r + WG_RADIUS - k][c] + (double)tile[r + WG_RADIUS + k][c]) * taps.w[k];
        mid[r][c] = (float)acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < WG_TILE * WG_TILE; e += 256) {  // axis 1
        const int r = e / WG_TILE, c = e - r * WG_TILE;
        const int y = y0 + r, x = x0 + c;
        if (y >= h || x >= w) continue;
        double acc = (double)mid[r][c + WG_RADIUS] * taps.w[0];
#pragma unroll
        for (int k = WG_RADIUS; k >= 1; --k) acc += ((double)mid[r][c + WG_RADIUS - k] + (double)mid[r][c + WG_RADIUS + k]) * taps.w[k];
        const float smooth = (float)acc;
        // numpy.linspace(-1, 1, n): arange(n) * (2 / (n - 1)) + (-1), the last element set to the stop value; n = 1 -> [-1]
        const int i = z == 0 ? x : y, n = z == 0 ? w : h;
        double lin = -1.0;
        if (n > 1) lin = i == n - 1 ? 1.0 : __dadd_rn(__dmul_rn((double)i, 2.0 / (double)(n - 1)), -1.0);
        out[((int64_t)z * h + y) * w + x] = (float)(lin + (double)smooth);
    }
}

// The source position of resize_bilinear_kernel (image.hip; ATen's area_pixel_compute_source_index, align_corners=False) for one axis:
// index of the first neighbour, of the second (clamped at the far edge) and the second one's weight.
__device__ __forceinline__ void bilinear_source(int o, float scale, int size, int& i0, int& i1, float& l) {
    float s = scale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, size - 1);
    i1 = i0 + (i0 < size - 1 ? 1 : 0);
    l = s - (float)i0;
}

// grid[oy][ox][z] from the planar two-component map [2][h][w]: resize_bilinear_kernel's coordinates and weights, the four-term blend
// summed in fp64 and rounded once
__global__ void __launch_bounds__(256) flow_warp_resize_kernel(const float* __restrict__ planar, float* __restrict__ grid, int h, int w,
                                                               int OH, int OW, float scale_h, float scale_w) {
    const int64_t total = (int64_t)OH * OW;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % OW), oy = (int)(e / OW);
        int y0, y1, x0, x1;
        float ly, lx;
        bilinear_source(oy, scale_h, h, y0, y1, ly);
        bilinear_source(ox, scale_w, w, x0, x1, lx);
        const double dly = ly, dlx = lx, dhy = 1.f - ly, dhx = 1.f - lx;
        float2 r;
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            const float* p = planar + (int64_t)z * h * w;
            const double v = dhy * (dhx * p[(int64_t)y0 * w + x0] + dlx * p[(int64_t)y0 * w + x1]) +
                             dly * (dhx * p[(int64_t)y1 * w + x0] + dlx * p[(int64_t)y1 * w + x1]);
            (z == 0 ? r.x : r.y) = (float)v;
        }
        reinterpret_cast<float2*>(grid)[e] = r;
    }
}

// One thread per output pixel: position and the four weights once (fp64 from the fp32 grid value: the position of a sample in a plane of
// hundreds of pixels keeps all of its fraction bits), then every channel's four taps.  Border padding: the position is clamped to
// [0, size - 1]; the second neighbour of a sample on the last row / column has weight 0 and is read at the clamped index.
// blend != null (h x w == H x W): init[n][c][oy][ox] = (1 - a) * blend + a * x at the output's own pixel, the temporal blend of the
// host loop, from the same pass over x; fp64 arithmetic, rounded once.
__global__ void __launch_bounds__(256) grid_sample_border_kernel(const float* __restrict__ x, const float* __restrict__ grid,
                                                                 float* __restrict__ y, int N, int C, int h, int w, int H, int W,
                                                                 const float* __restrict__ blend, double blend_a,
                                                                 float* __restrict__ init) {
    const int64_t plane_o = (int64_t)H * W, plane_i = (int64_t)h * w, total = (int64_t)N * plane_o;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = e / plane_o, o = e - n * plane_o;
        const float2 g = reinterpret_cast<const float2*>(grid)[e];
        double ix = (((double)g.x + 1.0) * (double)w - 1.0) * 0.5, iy = (((double)g.y + 1.0) * (double)h - 1.0) * 0.5;
        ix = fmin(fmax(ix, 0.0), (double)(w - 1));  // (a NaN position samples pixel 0: fmax returns the other operand)
        iy = fmin(fmax(iy, 0.0), (double)(h - 1));
        const int x0 = (int)ix, y0 = (int)iy;
        const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
        const double fx = ix - (double)x0, fy = iy - (double)y0;
        const double nw = (1.0 - fx) * (1.0 - fy), ne = fx * (1.0 - fy), sw = (1.0 - fx) * fy, se = fx * fy;
        const int64_t o00 = (int64_t)y0 * w + x0, o01 = (int64_t)y0 * w + x1, o10 = (int64_t)y1 * w + x0, o11 = (int64_t)y1 * w + x1;
        for (int c = 0; c < C; ++c) {
            const float* p = x + (n * C + c) * plane_i;
            y[(n * C + c) * plane_o + o] = (float)((double)p[o00] * nw + (double)p[o01] * ne + (double)p[o10] * sw + (double)p[o11] * se);
            if (blend) {
                const int64_t q = (n * C + c) * plane_o + o;
                init[q] = (float)((1.0 - blend_a) * (double)blend[q] + blend_a * (double)p[o]);
            }
        }
    }
}

// out[ch][oy][ox] = bilinear resize (resize_bilinear_kernel's arithmetic, fp32) of float(mask[y][x][ch]) / 255
__global__ void __launch_bounds__(256) mask_u8_resize_kernel(const unsigned char* __restrict__ mask, float* __restrict__ out, int h, int w,
                                                             int C, int OH, int OW, float scale_h, float scale_w) {
    const int64_t total = (int64_t)C * OH * OW;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(e % OW), oy = (int)((e / OW) % OH), ch = (int)(e / ((int64_t)OW * OH));
        int y0, y1, x0, x1;
        float ly, lx;
        bilinear_source(oy, scale_h, h, y0, y1, ly);
        bilinear_source(ox, scale_w, w, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float v00 = __fdiv_rn((float)mask[((int64_t)y0 * w + x0) * C + ch], 255.f), v01 = __fdiv_rn((float)mask[((int64_t)y0 * w + x1) * C + ch], 255.f);
        const float v10 = __fdiv_rn((float)mask[((int64_t)y1 * w + x0) * C + ch], 255.f), v11 = __fdiv_rn((float)mask[((int64_t)y1 * w + x1) * C + ch], 255.f);
        out[e] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
}

}  // namespace maua

using namespace maua;

extern "C" {

size_t maua_flow_warp_grid_workspace_bytes(int h, int w) {
    if (!conv_dims_ok(1, 2, h, w, 2, 0)) return 0;
    return (size_t)2 * (size_t)h * (size_t)w * sizeof(float);
}

int maua_flow_warp_grid(const float* flow_hw2, float* grid_hw2, int h, int w, int oh, int ow, void* workspace, size_t workspace_bytes,
                        maua_stream_t stream) {
    MAUA_REQUIRE(flow_hw2 && grid_hw2 && workspace, MAUA_E_INVAL, "flow_warp_grid: null pointer");
    MAUA_REQUIRE(conv_dims_ok(1, 2, h, w, 2, 0) && conv_dims_ok(1, 2, oh, ow, 2, 0), MAUA_E_INVAL, "flow_warp_grid: bad dims %d x %d -> %d x %d",
                 h, w, oh, ow);
    MAUA_REQUIRE(((uintptr_t)grid_hw2 & 7) == 0, MAUA_E_INVAL, "flow_warp_grid: the grid must be 8-byte aligned");
    MAUA_REQUIRE(workspace_bytes >= maua_flow_warp_grid_workspace_bytes(h, w), MAUA_E_WORKSPACE, "flow_warp_grid: workspace too small");
    const int tiles_x = (w + WG_TILE - 1) / WG_TILE, tiles_y = (h + WG_TILE - 1) / WG_TILE;
    MAUA_REQUIRE(tiles_y <= 65535, MAUA_E_UNSUPPORTED, "flow_warp_grid: %d rows", h);
    // scipy.ndimage._gaussian_kernel1d(sigma = 5, order 0, radius 20): exp(-0.5 / sigma^2 * x^2) / sum, in fp64
    GaussTaps taps;
    double sum = 0.0;
    for (int k = -WG_RADIUS; k <= WG_RADIUS; ++k) sum += exp(-0.5 / 25.0 * (double)(k * k));
    for (int k = 0; k <= WG_RADIUS; ++k) taps.w[k] = exp(-0.5 / 25.0 * (double)(k * k)) / sum;
    hipLaunchKernelGGL(flow_warp_smooth_kernel, dim3(tiles_x, tiles_y, 2), dim3(256), 0, (hipStream_t)stream, flow_hw2, (float*)workspace, h,
                       w, taps);
    int rc = check_launch("flow_warp_smooth_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(flow_warp_resize_kernel, dim3(reduce_blocks((int64_t)oh * ow, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, grid_hw2, h, w, oh, ow, (float)h / (float)oh, (float)w / (float)ow);
    return check_launch("flow_warp_resize_kernel");
}

int maua_grid_sample_border(const float* x, const float* grid, float* y, int n, int c, int h, int w, int oh, int ow, const float* blend,
                            double blend_a, float* init, maua_stream_t stream) {
    MAUA_REQUIRE(x && grid && y, MAUA_E_INVAL, "grid_sample_border: null pointer");
    MAUA_REQUIRE(conv_dims_ok(n, c, h, w, c, 0) && conv_dims_ok(n, c, oh, ow, c, 0), MAUA_E_INVAL, "grid_sample_border: bad dims");
    MAUA_REQUIRE(((uintptr_t)grid & 7) == 0, MAUA_E_INVAL, "grid_sample_border: the grid must be 8-byte aligned");
    MAUA_REQUIRE((blend == nullptr) == (init == nullptr), MAUA_E_INVAL, "grid_sample_border: blend and init go together");
    MAUA_REQUIRE(!blend || (h == oh && w == ow), MAUA_E_INVAL, "grid_sample_border: the fused blend needs %d x %d == %d x %d", h, w, oh, ow);
    MAUA_REQUIRE(!blend || isfinite(blend_a), MAUA_E_INVAL, "grid_sample_border: blend factor is not finite");
    hipLaunchKernelGGL(grid_sample_border_kernel, dim3(reduce_blocks((int64_t)n * oh * ow, 256)), dim3(256), 0, (hipStream_t)stream, x, grid,
                       y, n, c, h, w, oh, ow, blend, blend_a, init);
    return check_launch("grid_sample_border_kernel");
}

int maua_mask_u8_resize(const uint8_t* mask_hwc, float* out_chw, int h, int w, int c, int oh, int ow, maua_stream_t stream) {
    MAUA_REQUIRE(mask_hwc && out_chw, MAUA_E_INVAL, "mask_u8_resize: null pointer");
    MAUA_REQUIRE(conv_dims_ok(1, c, h, w, c, 0) && conv_dims_ok(1, c, oh, ow, c, 0) && c <= 4, MAUA_E_INVAL, "mask_u8_resize: bad dims");
    hipLaunchKernelGGL(mask_u8_resize_kernel, dim3(reduce_blocks((int64_t)c * oh * ow, 256)), dim3(256), 0, (hipStream_t)stream, mask_hwc,
                       out_chw, h, w, c, oh, ow, (float)h / (float)oh, (float)w / (float)ow);
    return check_launch("mask_u8_resize_kernel");
}

}  // extern "C"
