// Neural cellular automaton texture model (the reference's NCA_train.py / NCA_gen.py, CA.forward lines 154-186): one fused launch
// per CA step, its backward for backpropagation through time, and the finishing reduction of the parameter gradient.
// DESIGN.md section "Neural cellular automaton" has the layouts, the update-mask function and the reduction order.
//
// State x: (n, C, h, w) fp32.  Parameters: one flat fp32 buffer [w1 (HID x 4C)][b1 (HID)][w2 (C x HID)], the reference's
// Conv2d weights with the 1x1 taps dropped.  Perception channel 4c + f = channel c under filter f (ident, sobel_x, sobel_x^T,
// lap), circular padding.  Every product is an explicit fmaf chain in a fixed order and the file is compiled with contraction off,
// so the forward launch and the backward launch's recomputation of h and of the ReLU decisions agree bit for bit.
// Deterministic: no float atomics; the weight gradient goes through per-workgroup partial slots summed in fixed order.
// hipcc-flags: -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace maua {

namespace {

constexpr int FWD_THREADS = 256;
constexpr int FWD_MAX_BLOCKS = 4096;   // grid-stride beyond this: the weights are staged into LDS once per workgroup
constexpr int BWD_TILE = 64;           // pixels per backward tile = threads per backward workgroup
constexpr int BWD_MAX_BLOCKS = 1024;   // partial slots; tiles beyond this many fold into the same slots, in tile order
constexpr int RED_THREADS = 256;

bool dims_ok(int n, int h, int w) {
    return n > 0 && n <= (1 << 16) && h > 0 && h <= (1 << 14) && w > 0 && w <= (1 << 14) && (int64_t)n * h * w <= (1ll << 28);
}

bool pair_ok(int chn, int hidden) { return (chn == 12 && hidden == 96) || (chn == 16 && hidden == 128); }

int64_t param_count(int chn, int hidden) { return (int64_t)hidden * 4 * chn + hidden + (int64_t)chn * hidden; }

// ---- the update mask: a stateless function of (seed, step, b, y, x) -------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's output function
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint64_t launch_key(uint64_t seed, int64_t step) { return mix64(seed ^ mix64((uint64_t)step)); }

struct MaskArgs {
    const float* rate_map;  // (h, w) or null
    const float* mask;      // (n, h, w) explicit mask or null
    float rate;
    uint64_t key;
};

__device__ __forceinline__ float update_mask(const MaskArgs& ma, int b, int y, int x, int h, int w) {
    const int64_t pix = (int64_t)y * w + x;
    if (ma.mask) return ma.mask[(int64_t)b * h * w + pix];
    const float rate = ma.rate_map ? ma.rate_map[pix] : ma.rate;
    const uint64_t ctr = ((uint64_t)b << 40) | ((uint64_t)y << 20) | (uint64_t)x;
    const float u = (float)(uint32_t)(mix64(ma.key ^ ctr) >> 40) * 0x1p-24f;
    return floorf(u + rate);
}

// ---- the shared per-pixel pieces ----------------------------------------------------------------------------------------------
// p[4c + f] for the pixel (y, x) of image xb (C planes of h * w), circular neighbourhood
template <int C>
__device__ __forceinline__ void perceive(const float* __restrict__ xb, int h, int w, int y, int x, float* p) {
    const int64_t plane = (int64_t)h * w;
    const int ym = y == 0 ? h - 1 : y - 1, yp = y == h - 1 ? 0 : y + 1;
    const int xm = x == 0 ? w - 1 : x - 1, xp = x == w - 1 ? 0 : x + 1;
    const int64_t r0 = (int64_t)ym * w, r1 = (int64_t)y * w, r2 = (int64_t)yp * w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* q = xb + c * plane;
        const float a00 = q[r0 + xm], a01 = q[r0 + x], a02 = q[r0 + xp];
        const float a10 = q[r1 + xm], a11 = q[r1 + x], a12 = q[r1 + xp];
        const float a20 = q[r2 + xm], a21 = q[r2 + x], a22 = q[r2 + xp];
        p[4 * c + 0] = a11;
        p[4 * c + 1] = ((a02 - a00) + 2.0f * (a12 - a10)) + (a22 - a20);
        p[4 * c + 2] = ((a20 - a00) + 2.0f * (a21 - a01)) + (a22 - a02);
        p[4 * c + 3] = (((a00 + a02) + (a20 + a22)) + 2.0f * ((a01 + a21) + (a10 + a12))) - 12.0f * a11;
    }
}

// pre-activation a_j = b1[j] + sum_k w1[j][k] p[k], k ascending
template <int K>
__device__ __forceinline__ float hidden_pre(const float* __restrict__ w1row, float b, const float* p) {
    float a = b;
#pragma unroll
    for (int k = 0; k < K; ++k) a = fmaf(w1row[k], p[k], a);
    return a;
}

// LDS copy of the parameters: w1 [HID][4C], b1 [HID], w2 transposed to [HID][C]
template <int C, int HID>
__device__ __forceinline__ void stage_params(const float* __restrict__ params, float* sw1, float* sb1, float* sw2t) {
    constexpr int K = 4 * C;
    for (int i = threadIdx.x; i < HID * K; i += blockDim.x) sw1[i] = params[i];
    for (int i = threadIdx.x; i < HID; i += blockDim.x) sb1[i] = params[HID * K + i];
    for (int i = threadIdx.x; i < C * HID; i += blockDim.x) {
        const int c = i / HID, j = i - c * HID;
        sw2t[j * C + c] = params[HID * K + HID + i];
    }
}

// ---- forward: x_next = x + mask * W2 relu(W1 p(x) + b1) -----------------------------------------------------------------------
template <int C, int HID>
__global__ void __launch_bounds__(FWD_THREADS) nca_step_kernel(const float* __restrict__ xin, float* __restrict__ xout,
                                                               const float* __restrict__ params, int n, int h, int w, MaskArgs ma) {
    constexpr int K = 4 * C;
    __shared__ float sw1[HID * K];
    __shared__ float sb1[HID];
    __shared__ float sw2t[HID * C];
    stage_params<C, HID>(params, sw1, sb1, sw2t);
    __syncthreads();
    const int64_t plane = (int64_t)h * w, total = (int64_t)n * plane;
    for (int64_t pid = (int64_t)blockIdx.x * FWD_THREADS + threadIdx.x; pid < total; pid += (int64_t)gridDim.x * FWD_THREADS) {
        const int b = (int)(pid / plane);
        const int64_t pix = pid - (int64_t)b * plane;
        const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
        const float* xb = xin + (int64_t)b * C * plane;
        float p[K];
        perceive<C>(xb, h, w, y, x, p);
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0f;
        for (int j = 0; j < HID; ++j) {
            const float hj = fmaxf(hidden_pre<K>(sw1 + j * K, sb1[j], p), 0.0f);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = fmaf(sw2t[j * C + c], hj, acc[c]);
        }
        const float m = update_mask(ma, b, y, x, h, w);
        float* ob = xout + (int64_t)b * C * plane + pix;
#pragma unroll
        for (int c = 0; c < C; ++c) ob[c * plane] = xb[c * plane + pix] + acc[c] * m;
    }
}

// ---- backward, pass 1: per pixel dp = W1^T (relu'(a) . W2^T (mask g)) into dP, and the weight-gradient partials --------------
// LDS rows are padded by one float so that a thread walking its own row does not conflict with its neighbours.
template <int C, int HID>
constexpr int bwd_lds_floats() {
    return HID * 4 * C + HID + HID * C + BWD_TILE * ((HID + 1) + (4 * C + 1) + (C + 1));
}

template <int C, int HID>
__global__ void __launch_bounds__(BWD_TILE) nca_bwd_kernel(const float* __restrict__ xin, const float* __restrict__ g,
                                                           const float* __restrict__ params, float* __restrict__ dP,
                                                           float* __restrict__ part, int n, int h, int w, MaskArgs ma) {
    constexpr int K = 4 * C, P = HID * K + HID + C * HID;
    constexpr int SH = HID + 1, SP = K + 1, SM = C + 1;
    extern __shared__ float lds[];
    float* sw1 = lds;
    float* sb1 = sw1 + HID * K;
    float* sw2t = sb1 + HID;
    float* sH = sw2t + HID * C;  // h, then da, per pixel [BWD_TILE][SH]
    float* sP = sH + BWD_TILE * SH;
    float* sM = sP + BWD_TILE * SP;
    stage_params<C, HID>(params, sw1, sb1, sw2t);
    const int t = threadIdx.x;
    const int64_t plane = (int64_t)h * w, total = (int64_t)n * plane;
    const int64_t tiles = (total + BWD_TILE - 1) / BWD_TILE;
    float* mypart = part + (int64_t)blockIdx.x * P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();  // parameters staged / the previous tile's reductions done
        const int64_t pid = tile * BWD_TILE + t;
        const bool live = pid < total;
        int b = 0, y = 0, x = 0;
        int64_t pix = 0;
        float mg[C];
        if (live) {
            b = (int)(pid / plane);
            pix = pid - (int64_t)b * plane;
            y = (int)(pix / w);
            x = (int)(pix - (int64_t)y * w);
            float p[K];
            perceive<C>(xin + (int64_t)b * C * plane, h, w, y, x, p);
#pragma unroll
            for (int k = 0; k < K; ++k) sP[t * SP + k] = p[k];
            for (int j = 0; j < HID; ++j) sH[t * SH + j] = fmaxf(hidden_pre<K>(sw1 + j * K, sb1[j], p), 0.0f);
            const float m = update_mask(ma, b, y, x, h, w);
            const float* gb = g + (int64_t)b * C * plane + pix;
#pragma unroll
            for (int c = 0; c < C; ++c) mg[c] = m * gb[c * plane];
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) sP[t * SP + k] = 0.0f;
            for (int j = 0; j < HID; ++j) sH[t * SH + j] = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) mg[c] = 0.0f;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) sM[t * SM + c] = mg[c];
        __syncthreads();
        // dW2[c][j] += sum over the tile's pixels (ascending) of mg_c h_j
        for (int e = t; e < C * HID; e += BWD_TILE) {
            const int c = e / HID, j = e - c * HID;
            float s = 0.0f;
            for (int q = 0; q < BWD_TILE; ++q) s = fmaf(sM[q * SM + c], sH[q * SH + j], s);
            mypart[HID * K + HID + e] += s;
        }
        __syncthreads();
        // da_j = relu'(a_j) sum_c w2[c][j] mg_c (in place of h_j);  dp = W1^T da, j ascending
        {
            float dp[K];
#pragma unroll
            for (int k = 0; k < K; ++k) dp[k] = 0.0f;
            for (int j = 0; j < HID; ++j) {
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) s = fmaf(sw2t[j * C + c], mg[c], s);
                const float da = sH[t * SH + j] > 0.0f ? s : 0.0f;
                sH[t * SH + j] = da;
#pragma unroll
                for (int k = 0; k < K; ++k) dp[k] = fmaf(sw1[j * K + k], da, dp[k]);
            }
            if (live) {
                float* db = dP + (int64_t)b * K * plane + pix;
#pragma unroll
                for (int k = 0; k < K; ++k) db[k * plane] = dp[k];
            }
        }
        __syncthreads();
        // dW1[j][k] += sum_q da_j p_k ; db1[j] += sum_q da_j
        for (int e = t; e < HID * K; e += BWD_TILE) {
            const int j = e / K, k = e - j * K;
            float s = 0.0f;
            for (int q = 0; q < BWD_TILE; ++q) s = fmaf(sH[q * SH + j], sP[q * SP + k], s);
            mypart[e] += s;
        }
        for (int j = t; j < HID; j += BWD_TILE) {
            float s = 0.0f;
            for (int q = 0; q < BWD_TILE; ++q) s += sH[q * SH + j];
            mypart[HID * K + j] += s;
        }
    }
}

// ---- backward, pass 2: dx = g + perception^T(dP), the same circular neighbourhood read the other way ----------------------------
template <int C>
__global__ void __launch_bounds__(256) nca_bwd_gather_kernel(const float* __restrict__ dP, const float* g, float* dx, int n, int h,
                                                             int w) {
    const int64_t plane = (int64_t)h * w, total = (int64_t)n * C * plane;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t bc = i / plane, pix = i - bc * plane;
    const int b = (int)(bc / C), c = (int)(bc - (int64_t)b * C);
    const int y = (int)(pix / w), x = (int)(pix - (int64_t)y * w);
    // p(q) = sum_{i,j} K[i][j] x(q + (i - 1, j - 1))  =>  dx(r) = sum_{i,j} K[i][j] dp(r - (i - 1, j - 1))
    const int ym = y == 0 ? h - 1 : y - 1, yp = y == h - 1 ? 0 : y + 1;
    const int xm = x == 0 ? w - 1 : x - 1, xp = x == w - 1 ? 0 : x + 1;
    const int64_t rs[3] = {(int64_t)yp * w, (int64_t)y * w, (int64_t)ym * w};  // row of tap row i = 0, 1, 2
    const int cs[3] = {xp, x, xm};
    const float* d = dP + ((int64_t)b * 4 * C + 4 * c) * plane;
    const float* d1 = d + plane;
    const float* d2 = d1 + plane;
    const float* d3 = d2 + plane;
    constexpr float SX[3][3] = {{-1.f, 0.f, 1.f}, {-2.f, 0.f, 2.f}, {-1.f, 0.f, 1.f}};
    constexpr float LP[3][3] = {{1.f, 2.f, 1.f}, {2.f, -12.f, 2.f}, {1.f, 2.f, 1.f}};
    float acc = d[rs[1] + cs[1]];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int64_t o = rs[a] + cs[e];
            if (SX[a][e] != 0.f) acc = fmaf(SX[a][e], d1[o], acc);
            if (SX[e][a] != 0.f) acc = fmaf(SX[e][a], d2[o], acc);
            acc = fmaf(LP[a][e], d3[o], acc);
        }
    }
    dx[i] = g[i] + acc;
}

// ---- finishing: grad[e] = sum over slots (ascending) of part[slot][e], fp64 accumulation -----------------------------------------
__global__ void __launch_bounds__(RED_THREADS) nca_reduce_kernel(const float* __restrict__ part, float* __restrict__ grad, int slots,
                                                                 int count) {
    const int e = blockIdx.x * RED_THREADS + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int k = 0; k < slots; ++k) s += (double)part[(int64_t)k * count + e];
    grad[e] = (float)s;
}

// grad of each of the three tensors /= (its L2 norm + 1e-8): one workgroup per tensor, fixed-order tree in fp64
__global__ void __launch_bounds__(RED_THREADS) nca_grad_normalize_kernel(float* grad, int n_w1, int n_b1, int n_w2) {
    __shared__ double red[RED_THREADS];
    const int off = blockIdx.x == 0 ? 0 : blockIdx.x == 1 ? n_w1 : n_w1 + n_b1;
    const int cnt = blockIdx.x == 0 ? n_w1 : blockIdx.x == 1 ? n_b1 : n_w2;
    float* gp = grad + off;
    double s = 0.0;
    for (int i = threadIdx.x; i < cnt; i += RED_THREADS) s += (double)gp[i] * (double)gp[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = RED_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    const float den = (float)sqrt(red[0]) + 1e-8f;
    for (int i = threadIdx.x; i < cnt; i += RED_THREADS) gp[i] = gp[i] / den;
}

template <int C, int HID>
int launch_step(const float* x, float* out, const float* params, int n, int h, int w, const MaskArgs& ma, hipStream_t st) {
    const int64_t total = (int64_t)n * h * w;
    const int64_t blocks = (total + FWD_THREADS - 1) / FWD_THREADS;
    nca_step_kernel<C, HID><<<(int)(blocks < FWD_MAX_BLOCKS ? blocks : FWD_MAX_BLOCKS), FWD_THREADS, 0, st>>>(x, out, params, n, h, w,
                                                                                                           ma);
    return check_launch("nca_step");
}

int64_t bwd_slots(int n, int h, int w) {
    const int64_t tiles = ((int64_t)n * h * w + BWD_TILE - 1) / BWD_TILE;
    return tiles < BWD_MAX_BLOCKS ? tiles : BWD_MAX_BLOCKS;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

template <int C, int HID>
int launch_bwd(const float* x, const float* g, float* dx, const float* params, int n, int h, int w, const MaskArgs& ma, float* part,
               float* dP, hipStream_t st) {
    static unsigned long long served = 0;  // (once per device)
    constexpr int lds = bwd_lds_floats<C, HID>() * (int)sizeof(float);
    if (opt_in_dynamic_lds(reinterpret_cast<const void*>(nca_bwd_kernel<C, HID>), lds, &served) != hipSuccess)
        return check_launch("nca_step_bwd (LDS opt-in)");
    nca_bwd_kernel<C, HID><<<(int)bwd_slots(n, h, w), BWD_TILE, lds, st>>>(x, g, params, dP, part, n, h, w, ma);
    int rc = check_launch("nca_step_bwd");
    if (rc != MAUA_OK) return rc;
    const int64_t total = (int64_t)n * C * h * w;
    nca_bwd_gather_kernel<C><<<(int)((total + 255) / 256), 256, 0, st>>>(dP, g, dx, n, h, w);
    return check_launch("nca_step_bwd (gather)");
}

}  // namespace
}  // namespace maua

using namespace maua;

extern "C" int maua_nca_supported(int n, int chn, int hidden, int h, int w) { return dims_ok(n, h, w) && pair_ok(chn, hidden); }

extern "C" int64_t maua_nca_param_count(int chn, int hidden) { return pair_ok(chn, hidden) ? param_count(chn, hidden) : 0; }

extern "C" int maua_nca_step(const float* x, float* out, const float* params, int n, int chn, int hidden, int h, int w, float rate,
                             const float* rate_map, const float* mask, uint64_t seed, int64_t step, maua_stream_t stream) {
    MAUA_REQUIRE(x && out && params, MAUA_E_INVAL, "nca_step: null pointer");
    MAUA_REQUIRE(x != out, MAUA_E_INVAL, "nca_step: out must not alias x");
    MAUA_REQUIRE(dims_ok(n, h, w), MAUA_E_INVAL, "nca_step: bad size n=%d h=%d w=%d", n, h, w);
    MAUA_REQUIRE(pair_ok(chn, hidden), MAUA_E_UNSUPPORTED, "nca_step: chn/hidden %d/%d not built (12/96, 16/128)", chn, hidden);
    MAUA_REQUIRE(step >= 0, MAUA_E_INVAL, "nca_step: negative step");
    const MaskArgs ma{rate_map, mask, rate, launch_key(seed, step)};
    hipStream_t st = (hipStream_t)stream;
    if (chn == 12) return launch_step<12, 96>(x, out, params, n, h, w, ma, st);
    return launch_step<16, 128>(x, out, params, n, h, w, ma, st);
}

extern "C" size_t maua_nca_bwd_workspace_bytes(int n, int chn, int hidden, int h, int w) {
    if (!dims_ok(n, h, w) || !pair_ok(chn, hidden)) return 0;
    return align256((size_t)bwd_slots(n, h, w) * param_count(chn, hidden) * sizeof(float)) +
           align256((size_t)n * 4 * chn * h * w * sizeof(float));
}

extern "C" int maua_nca_step_bwd(const float* x, const float* g, float* dx, const float* params, int n, int chn, int hidden, int h, int w,
                                 float rate, const float* rate_map, const float* mask, uint64_t seed, int64_t step, int first,
                                 void* workspace, size_t workspace_bytes, maua_stream_t stream) {
    MAUA_REQUIRE(x && g && dx && params && workspace, MAUA_E_INVAL, "nca_step_bwd: null pointer");
    MAUA_REQUIRE(dx != x, MAUA_E_INVAL, "nca_step_bwd: dx must not alias x");
    MAUA_REQUIRE(dims_ok(n, h, w), MAUA_E_INVAL, "nca_step_bwd: bad size n=%d h=%d w=%d", n, h, w);
    MAUA_REQUIRE(pair_ok(chn, hidden), MAUA_E_UNSUPPORTED, "nca_step_bwd: chn/hidden %d/%d not built (12/96, 16/128)", chn, hidden);
    MAUA_REQUIRE(step >= 0, MAUA_E_INVAL, "nca_step_bwd: negative step");
    const size_t need = maua_nca_bwd_workspace_bytes(n, chn, hidden, h, w);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "nca_step_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
    const MaskArgs ma{rate_map, mask, rate, launch_key(seed, step)};
    hipStream_t st = (hipStream_t)stream;
    float* part = static_cast<float*>(workspace);
    const size_t part_bytes = align256((size_t)bwd_slots(n, h, w) * param_count(chn, hidden) * sizeof(float));
    float* dP = reinterpret_cast<float*>(static_cast<char*>(workspace) + part_bytes);
    if (first) {
        const hipError_t rc = hipMemsetAsync(part, 0, part_bytes, st);
        MAUA_REQUIRE(rc == hipSuccess, (int)rc, "nca_step_bwd: hipMemsetAsync: %s", hipGetErrorString(rc));
    }
    if (chn == 12) return launch_bwd<12, 96>(x, g, dx, params, n, h, w, ma, part, dP, st);
    return launch_bwd<16, 128>(x, g, dx, params, n, h, w, ma, part, dP, st);
}

extern "C" int maua_nca_grad_finish(float* grad, int n, int chn, int hidden, int h, int w, const void* workspace, size_t workspace_bytes,
                                    int normalize, maua_stream_t stream) {
    MAUA_REQUIRE(grad && workspace, MAUA_E_INVAL, "nca_grad_finish: null pointer");
    MAUA_REQUIRE(dims_ok(n, h, w), MAUA_E_INVAL, "nca_grad_finish: bad size n=%d h=%d w=%d", n, h, w);
    MAUA_REQUIRE(pair_ok(chn, hidden), MAUA_E_UNSUPPORTED, "nca_grad_finish: chn/hidden %d/%d not built", chn, hidden);
    const size_t need = maua_nca_bwd_workspace_bytes(n, chn, hidden, h, w);
    MAUA_REQUIRE(workspace_bytes >= need, MAUA_E_WORKSPACE, "nca_grad_finish: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int count = (int)param_count(chn, hidden);
    nca_reduce_kernel<<<(count + RED_THREADS - 1) / RED_THREADS, RED_THREADS, 0, st>>>(static_cast<const float*>(workspace), grad,
                                                                                       (int)bwd_slots(n, h, w), count);
    int rc = check_launch("nca_grad_finish");
    if (rc != MAUA_OK || !normalize) return rc;
    nca_grad_normalize_kernel<<<3, RED_THREADS, 0, st>>>(grad, hidden * 4 * chn, hidden, chn * hidden);
    return check_launch("nca_grad_finish (normalize)");
}
