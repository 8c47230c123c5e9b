// Scale-space motion compensation of ScaleSpaceFlow (models/video/google.py: gaussian_volume + warp_volume).
// fp32 throughout; images are dense NCHW planes [planes][H][W], the volume is [N][C][D][H][W] with D = levels + 1.
//
// volume forward   level 0 = x (copy).  b_1 = blur(x) is level 1.  For l >= 2: b_l = blur(pool2x2(b_{l-1})) in one
//                  launch (the 2x2 average is taken in the tile load), then l - 1 bilinear x2 steps (align_corners =
//                  false: weights 1/4, 3/4, index clamp at the borders) that ping-pong in the workspace; the last
//                  step writes the level's slice of the volume.  The blur is separable (row pass, column pass through
//                  an LDS tile); the replicate border is a clamp of the load index, so a level smaller than the halo
//                  (a 1x1 level under a 5-pixel halo) needs nothing special.
// volume backward  the exact adjoints in gather form, no atomics: db_L = up^T ... up^T dvol_L; then for l = L .. 2:
//                  db_{l-1} = (up^T)^(l-2) dvol_{l-1} + pool^T blur^T db_l; dx = dvol_0 + blur^T db_1.  blur^T folds the
//                  taps that the clamp sent to an edge pixel onto that pixel (prefix / suffix sums of the taps).
// warp forward     one thread per output pixel, all C channels: trilinear sample of the volume at
//                  ix = w + flow_x W / 2, iy = h + flow_y H / 2, iz = ((s + 1) D - 1) / 2, each clamped to its axis
//                  (grid_sample, padding_mode = "border", align_corners = false).  Optional second output
//                  x_res = x_cur - x_pred.
// warp backward    d_motion from the corners' weight derivatives (zero where the coordinate was clamped); d_volume in
//                  a launch of its own with fp32 vector atomic adds into a zeroed buffer (its low bits depend on the
//                  order of the adds).
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace cai {

constexpr int SSF_MAX_TAPS = 31;
constexpr int SSF_MAX_R = SSF_MAX_TAPS / 2;
constexpr int SSF_TILE = 32;
constexpr int SSF_IN = SSF_TILE + 2 * SSF_MAX_R;   // 62

struct ssf_taps {
    float g[SSF_MAX_TAPS];     // the normalised taps
    float pre[SSF_MAX_TAPS];   // pre[k] = g[0] + .. + g[k]
    float suf[SSF_MAX_TAPS];   // suf[k] = g[k] + .. + g[K - 1]
    float total;
    int32_t K;
};

// dst[p][h][w] = src[p][h][w] for dense [H][W] planes with their own plane strides
__global__ __launch_bounds__(256) void ssf_copy_kernel(const float* __restrict__ src, int64_t src_ps,
                                                       float* __restrict__ dst, int64_t dst_ps, int64_t planes,
                                                       int64_t hw) {
    const int64_t n = planes * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i / hw, r = i - p * hw;
        dst[p * dst_ps + r] = src[p * src_ps + r];
    }
}

// dst[p][H][W] = blur(in), in = src (POOL = 0, [H][W]) or the 2x2 average of src (POOL = 1, src is [2H][2W]).
// One block per 32 x 32 output tile of one plane.
template <int POOL>
__global__ __launch_bounds__(256) void ssf_blur_kernel(const float* __restrict__ src, int64_t src_ps,
                                                       float* __restrict__ dst, int64_t dst_ps, int H, int W,
                                                       int tiles_x, int tiles, const ssf_taps t) {
    __shared__ float g[SSF_MAX_TAPS];
    __shared__ float raw[SSF_IN][SSF_IN + 1];
    __shared__ float hp[SSF_IN][SSF_TILE + 1];
    const int K = t.K, R = K >> 1, IN = SSF_TILE + 2 * R;
    const int p = blockIdx.x / tiles, tt = blockIdx.x - p * tiles;
    const int y0 = (tt / tiles_x) * SSF_TILE, x0 = (tt % tiles_x) * SSF_TILE;
    if (threadIdx.x < K) g[threadIdx.x] = t.g[threadIdx.x];
    const float* s = src + (int64_t)p * src_ps;
    for (int i = threadIdx.x; i < IN * IN; i += 256) {
        const int r = i / IN, c = i - r * IN;
        const int y = min(max(y0 + r - R, 0), H - 1), x = min(max(x0 + c - R, 0), W - 1);
        float v;
        if (POOL) {
            const float* q = s + (int64_t)(2 * y) * (2 * W) + 2 * x;
            v = ((q[0] + q[1]) + (q[2 * W] + q[2 * W + 1])) * 0.25f;
        } else {
            v = s[(int64_t)y * W + x];
        }
        raw[r][c] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < IN * SSF_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = fmaf(g[k], raw[r][j + k], a);
        hp[r][j] = a;
    }
    __syncthreads();
    float* d = dst + (int64_t)p * dst_ps;
    for (int i = threadIdx.x; i < SSF_TILE * SSF_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        if (y0 + r < H && x0 + j < W) {
            float a = 0.f;
            for (int k = 0; k < K; ++k) a = fmaf(g[k], hp[r + k][j], a);
            d[(int64_t)(y0 + r) * W + x0 + j] = a;
        }
    }
}

// bilinear x2 (align_corners = false): src [Hi][Wi] -> dst [2 Hi][2 Wi]
__global__ __launch_bounds__(256) void ssf_up2_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                      int64_t dst_ps, int64_t planes, int Hi, int Wi) {
    const int Ho = 2 * Hi, Wo = 2 * Wi;
    const int64_t n = planes * Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % Wo), h = (int)((i / Wo) % Ho);
        const int64_t p = i / ((int64_t)Wo * Ho);
        // even h: rows h/2 - 1 (1/4) and h/2 (3/4); odd h: rows (h-1)/2 (3/4) and (h+1)/2 (1/4)
        const int ya = max((h >> 1) - 1 + (h & 1), 0), yb = min((h >> 1) + (h & 1), Hi - 1);
        const int xa = max((w >> 1) - 1 + (w & 1), 0), xb = min((w >> 1) + (w & 1), Wi - 1);
        const float wya = (h & 1) ? 0.75f : 0.25f, wyb = 1.f - wya;
        const float wxa = (w & 1) ? 0.75f : 0.25f, wxb = 1.f - wxa;
        const float* s = src + p * (int64_t)Hi * Wi;
        const float top = wxa * s[(int64_t)ya * Wi + xa] + wxb * s[(int64_t)ya * Wi + xb];
        const float bot = wxa * s[(int64_t)yb * Wi + xa] + wxb * s[(int64_t)yb * Wi + xb];
        dst[p * dst_ps + (int64_t)h * Wo + w] = wya * top + wyb * bot;
    }
}

// the 1-D adjoint of the x2 step: input sample i collects outputs 2i - 1 .. 2i + 2 with weights 1/4, 3/4, 3/4, 1/4;
// the clamp sends the missing neighbour's weight of the first / last output back to the edge sample
__device__ __forceinline__ void up2t_weights(int i, int n, float (&w)[4]) {
    w[0] = i > 0 ? 0.25f : 0.f;
    w[1] = i > 0 ? 0.75f : 1.f;
    w[2] = i < n - 1 ? 0.75f : 1.f;
    w[3] = i < n - 1 ? 0.25f : 0.f;
}

// dst[Hi][Wi] = (UP ? up2^T g : g) + (pool ? pool^T: 1/4 pool[h / 2][w / 2] : 0); g is [2 Hi][2 Wi] (UP) or [Hi][Wi]
template <int UP>
__global__ __launch_bounds__(256) void ssf_up2t_kernel(const float* __restrict__ g, int64_t g_ps,
                                                       const float* __restrict__ pool, float* __restrict__ dst,
                                                       int64_t planes, int Hi, int Wi) {
    const int64_t n = planes * Hi * Wi;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % Wi), h = (int)((i / Wi) % Hi);
        const int64_t p = i / ((int64_t)Wi * Hi);
        const float* s = g + p * g_ps;
        float a;
        if (UP) {
            float wy[4], wx[4];
            up2t_weights(h, Hi, wy);
            up2t_weights(w, Wi, wx);
            const int Wo = 2 * Wi;
            a = 0.f;
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) {
                const int y = min(max(2 * h - 1 + dy, 0), 2 * Hi - 1);   // weight 0 where the clamp acts
                float r = 0.f;
#pragma unroll
                for (int dx = 0; dx < 4; ++dx) {
                    const int x = min(max(2 * w - 1 + dx, 0), Wo - 1);
                    r = fmaf(wx[dx], s[(int64_t)y * Wo + x], r);
                }
                a = fmaf(wy[dy], r, a);
            }
        } else {
            a = s[(int64_t)h * Wi + w];
        }
        if (pool) a += 0.25f * pool[p * (int64_t)(Hi >> 1) * (Wi >> 1) + (int64_t)(h >> 1) * (Wi >> 1) + (w >> 1)];
        dst[i] = a;
    }
}

// weight of output i = y - R + dk in the adjoint at input y of an axis of n samples (table index K - 1 - dk)
__device__ __forceinline__ float blurt_w(const float* g, const float* pre, const float* suf, float total, int y,
                                         int n, int idx) {
    const bool lo = y == 0, hi = y == n - 1;
    return lo ? (hi ? total : pre[idx]) : (hi ? suf[idx] : g[idx]);
}

// dst[p][H][W] = (add ? add : 0) + blur^T(g); g, dst dense [H][W] planes, add with its own plane stride
__global__ __launch_bounds__(256) void ssf_blurt_kernel(const float* __restrict__ gin, const float* __restrict__ add,
                                                        int64_t add_ps, float* __restrict__ dst, int H, int W,
                                                        int tiles_x, int tiles, const ssf_taps t) {
    __shared__ float g[SSF_MAX_TAPS], pre[SSF_MAX_TAPS], suf[SSF_MAX_TAPS];
    __shared__ float raw[SSF_IN][SSF_IN + 1];
    __shared__ float hp[SSF_IN][SSF_TILE + 1];
    const int K = t.K, R = K >> 1, IN = SSF_TILE + 2 * R;
    const int p = blockIdx.x / tiles, tt = blockIdx.x - p * tiles;
    const int y0 = (tt / tiles_x) * SSF_TILE, x0 = (tt % tiles_x) * SSF_TILE;
    if (threadIdx.x < K) {
        g[threadIdx.x] = t.g[threadIdx.x];
        pre[threadIdx.x] = t.pre[threadIdx.x];
        suf[threadIdx.x] = t.suf[threadIdx.x];
    }
    const float total = t.total;
    const float* s = gin + (int64_t)p * H * W;
    for (int i = threadIdx.x; i < IN * IN; i += 256) {
        const int r = i / IN, c = i - r * IN;
        const int y = y0 + r - R, x = x0 + c - R;
        raw[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? s[(int64_t)y * W + x] : 0.f;
    }
    __syncthreads();
    // with a single sample on the axis only output 0 exists, at dk = R
    for (int i = threadIdx.x; i < IN * SSF_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        const int x = x0 + j;
        float a = 0.f;
        if (x < W) {
            if (W == 1) {
                a = total * raw[r][j + R];
            } else {
                for (int dk = 0; dk < K; ++dk) a = fmaf(blurt_w(g, pre, suf, total, x, W, K - 1 - dk), raw[r][j + dk], a);
            }
        }
        hp[r][j] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SSF_TILE * SSF_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        const int y = y0 + r, x = x0 + j;
        if (y < H && x < W) {
            float a = 0.f;
            if (H == 1) {
                a = total * hp[r + R][j];
            } else {
                for (int dk = 0; dk < K; ++dk) a = fmaf(blurt_w(g, pre, suf, total, y, H, K - 1 - dk), hp[r + dk][j], a);
            }
            if (add) a += add[(int64_t)p * add_ps + (int64_t)y * W + x];
            dst[(int64_t)p * H * W + (int64_t)y * W + x] = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// warp
// ---------------------------------------------------------------------------------------------------------
struct ssf_coord {
    int i0, i1;
    float f;       // weight of i1
    float live;    // 1 where the coordinate was not clamped (its derivative passes), else 0
};

__device__ __forceinline__ ssf_coord ssf_axis(float v, int n) {
    ssf_coord c;
    const float top = (float)(n - 1);
    c.live = (v > 0.f && v < top) ? 1.f : 0.f;
    v = fminf(fmaxf(v, 0.f), top);
    const float fl = floorf(v);
    c.i0 = (int)fl;
    c.i1 = min(c.i0 + 1, n - 1);   // weight 0 where the clamp acts
    c.f = v - fl;
    return c;
}

struct ssf_warp_args {
    const float* vol;      // [N][C][D][H][W]
    const float* motion;   // [N][3][H][W] through strides
    int64_t m_sn, m_sc, m_sh, m_sw;
    int32_t N, C, D, H, W;
};

__device__ __forceinline__ void ssf_sample_pos(const ssf_warp_args& a, int n, int h, int w, ssf_coord& cx,
                                               ssf_coord& cy, ssf_coord& cz) {
    const float* m = a.motion + n * a.m_sn + h * a.m_sh + w * a.m_sw;
    const float fx = m[0], fy = m[a.m_sc], sc = m[2 * a.m_sc];
    cx = ssf_axis((float)w + fx * (0.5f * (float)a.W), a.W);
    cy = ssf_axis((float)h + fy * (0.5f * (float)a.H), a.H);
    cz = ssf_axis(((sc + 1.f) * (float)a.D - 1.f) * 0.5f, a.D);
}

__global__ __launch_bounds__(256) void ssf_warp_fwd_kernel(const ssf_warp_args a, float* __restrict__ out,
                                                           const float* __restrict__ x_cur, float* __restrict__ x_res) {
    const int64_t hw = (int64_t)a.H * a.W, npix = a.N * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / hw);
        const int64_t r = i - n * hw;
        const int h = (int)(r / a.W), w = (int)(r - (int64_t)h * a.W);
        ssf_coord cx, cy, cz;
        ssf_sample_pos(a, n, h, w, cx, cy, cz);
        const int64_t o00 = (cz.i0 * (int64_t)a.H + cy.i0) * a.W, o01 = (cz.i0 * (int64_t)a.H + cy.i1) * a.W;
        const int64_t o10 = (cz.i1 * (int64_t)a.H + cy.i0) * a.W, o11 = (cz.i1 * (int64_t)a.H + cy.i1) * a.W;
        const float wx1 = cx.f, wx0 = 1.f - cx.f, wy1 = cy.f, wy0 = 1.f - cy.f, wz1 = cz.f, wz0 = 1.f - cz.f;
        for (int c = 0; c < a.C; ++c) {
            const float* v = a.vol + ((int64_t)n * a.C + c) * a.D * hw;
            const float r00 = wx0 * v[o00 + cx.i0] + wx1 * v[o00 + cx.i1];
            const float r01 = wx0 * v[o01 + cx.i0] + wx1 * v[o01 + cx.i1];
            const float r10 = wx0 * v[o10 + cx.i0] + wx1 * v[o10 + cx.i1];
            const float r11 = wx0 * v[o11 + cx.i0] + wx1 * v[o11 + cx.i1];
            const float val = wz0 * (wy0 * r00 + wy1 * r01) + wz1 * (wy0 * r10 + wy1 * r11);
            const int64_t o = ((int64_t)n * a.C + c) * hw + r;
            out[o] = val;
            if (x_res) x_res[o] = x_cur[o] - val;
        }
    }
}

// g = g_pred - g_res (either nullable); d_motion [N][3][H][W] dense (nullable); d_vol zeroed [N][C][D][H][W] (nullable)
template <int DVOL>
__global__ __launch_bounds__(256) void ssf_warp_bwd_kernel(const ssf_warp_args a, const float* __restrict__ g_pred,
                                                           const float* __restrict__ g_res, float* __restrict__ d_motion,
                                                           float* __restrict__ d_vol) {
    const int64_t hw = (int64_t)a.H * a.W, npix = a.N * hw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / hw);
        const int64_t r = i - n * hw;
        const int h = (int)(r / a.W), w = (int)(r - (int64_t)h * a.W);
        ssf_coord cx, cy, cz;
        ssf_sample_pos(a, n, h, w, cx, cy, cz);
        const int64_t o00 = (cz.i0 * (int64_t)a.H + cy.i0) * a.W, o01 = (cz.i0 * (int64_t)a.H + cy.i1) * a.W;
        const int64_t o10 = (cz.i1 * (int64_t)a.H + cy.i0) * a.W, o11 = (cz.i1 * (int64_t)a.H + cy.i1) * a.W;
        const float wx1 = cx.f, wx0 = 1.f - cx.f, wy1 = cy.f, wy0 = 1.f - cy.f, wz1 = cz.f, wz0 = 1.f - cz.f;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int c = 0; c < a.C; ++c) {
            const int64_t o = ((int64_t)n * a.C + c) * hw + r;
            const float g = (g_pred ? g_pred[o] : 0.f) - (g_res ? g_res[o] : 0.f);
            const int64_t vb = ((int64_t)n * a.C + c) * a.D * hw;
            if (DVOL) {
                float* v = d_vol + vb;
                const float w00 = g * wz0 * wy0, w01 = g * wz0 * wy1, w10 = g * wz1 * wy0, w11 = g * wz1 * wy1;
                if (w00 * wx0 != 0.f) unsafeAtomicAdd(v + o00 + cx.i0, w00 * wx0);
                if (w00 * wx1 != 0.f) unsafeAtomicAdd(v + o00 + cx.i1, w00 * wx1);
                if (w01 * wx0 != 0.f) unsafeAtomicAdd(v + o01 + cx.i0, w01 * wx0);
                if (w01 * wx1 != 0.f) unsafeAtomicAdd(v + o01 + cx.i1, w01 * wx1);
                if (w10 * wx0 != 0.f) unsafeAtomicAdd(v + o10 + cx.i0, w10 * wx0);
                if (w10 * wx1 != 0.f) unsafeAtomicAdd(v + o10 + cx.i1, w10 * wx1);
                if (w11 * wx0 != 0.f) unsafeAtomicAdd(v + o11 + cx.i0, w11 * wx0);
                if (w11 * wx1 != 0.f) unsafeAtomicAdd(v + o11 + cx.i1, w11 * wx1);
            } else {
                const float* v = a.vol + vb;
                const float v000 = v[o00 + cx.i0], v001 = v[o00 + cx.i1], v010 = v[o01 + cx.i0], v011 = v[o01 + cx.i1];
                const float v100 = v[o10 + cx.i0], v101 = v[o10 + cx.i1], v110 = v[o11 + cx.i0], v111 = v[o11 + cx.i1];
                const float dx = wz0 * (wy0 * (v001 - v000) + wy1 * (v011 - v010))
                               + wz1 * (wy0 * (v101 - v100) + wy1 * (v111 - v110));
                const float dy = wz0 * (wx0 * (v010 - v000) + wx1 * (v011 - v001))
                               + wz1 * (wx0 * (v110 - v100) + wx1 * (v111 - v101));
                const float dz = wy0 * (wx0 * (v100 - v000) + wx1 * (v101 - v001))
                               + wy1 * (wx0 * (v110 - v010) + wx1 * (v111 - v011));
                gx = fmaf(g, dx, gx);
                gy = fmaf(g, dy, gy);
                gz = fmaf(g, dz, gz);
            }
        }
        if (!DVOL) {
            float* d = d_motion + (int64_t)n * 3 * hw + r;
            d[0] = gx * cx.live * (0.5f * (float)a.W);
            d[hw] = gy * cy.live * (0.5f * (float)a.H);
            d[2 * hw] = gz * cz.live * (0.5f * (float)a.D);
        }
    }
}

static int ssf_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(16384, (n + 255) / 256)); }

// the reference's kernel size 2 ceil(3 sigma) + 1 and its normalised taps
static int ssf_make_taps(float sigma, ssf_taps* t) {
    if (!(sigma > 0.f)) return 0;
    const int K = 2 * (int)std::ceil(3.0 * (double)sigma) + 1;
    if (K > SSF_MAX_TAPS) return K;
    double e[SSF_MAX_TAPS], sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double x = (k - (K - 1) / 2.0) / (double)sigma;
        e[k] = std::exp(-0.5 * x * x);
        sum += e[k];
    }
    memset(t, 0, sizeof(*t));
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        t->g[k] = (float)(e[k] / sum);
        acc += e[k] / sum;
        t->pre[k] = (float)acc;
    }
    acc = 0.0;
    for (int k = K - 1; k >= 0; --k) {
        acc += e[k] / sum;
        t->suf[k] = (float)acc;
    }
    t->total = 1.f;
    t->K = K;
    return K;
}

static int ssf_check_shape(const char* what, int32_t planes, int32_t H, int32_t W, int32_t levels) {
    CAI_CHECK_ARG(levels >= 1 && levels <= 12, "%s: levels %d outside 1..12", what, levels);
    CAI_CHECK_ARG(planes >= 1 && H >= 1 && W >= 1, "%s: bad shape %d x %d x %d", what, planes, H, W);
    const int m = 1 << (levels - 1);
    CAI_CHECK_ARG(H % m == 0 && W % m == 0, "%s: H = %d and W = %d must be multiples of 2^(levels-1) = %d", what, H, W,
                  m);
    CAI_CHECK_ARG((int64_t)planes * (levels + 1) * H * W < (1ll << 40), "%s: volume too large", what);
    return CAI_OK;
}

}  // namespace cai

using namespace cai;

extern "C" {

size_t cai_ssf_workspace_bytes(int32_t planes, int32_t H, int32_t W, int32_t levels) {
    if (ssf_check_shape("ssf_workspace_bytes", planes, H, W, levels) != CAI_OK) return 0;
    return (size_t)2 * planes * H * W * sizeof(float);
}

int cai_ssf_volume_fwd(const float* x, int32_t planes, int32_t H, int32_t W, float sigma, int32_t levels,
                       float* volume, void* workspace, size_t ws_bytes, void* stream) {
    int rc = ssf_check_shape("ssf_volume_fwd", planes, H, W, levels);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(x && volume && workspace, "ssf_volume_fwd: null pointer");
    ssf_taps taps;
    const int K = ssf_make_taps(sigma, &taps);
    CAI_CHECK_ARG(K >= 1 && K <= SSF_MAX_TAPS, "ssf_volume_fwd: sigma %g gives %d taps (1..%d supported)", (double)sigma,
                  K, SSF_MAX_TAPS);
    if (ws_bytes < cai_ssf_workspace_bytes(planes, H, W, levels)) {
        set_error("ssf_volume_fwd: workspace of %zu bytes is too small", ws_bytes);
        return CAI_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    const int64_t hw = (int64_t)H * W, vps = (int64_t)(levels + 1) * hw, q = (int64_t)planes * hw / 4;
    float* ws = (float*)workspace;
    float* bbuf[2] = {ws, ws + q};          // b_l of consecutive levels
    float* ubuf[2] = {ws + 2 * q, ws + 3 * q};   // the x2 chain
    hipLaunchKernelGGL(ssf_copy_kernel, dim3(ssf_grid(planes * hw)), dim3(256), 0, st, x, hw, volume, vps,
                       (int64_t)planes, hw);
    auto tiles_of = [](int h, int w, int& tx) {
        tx = (w + SSF_TILE - 1) / SSF_TILE;
        return tx * ((h + SSF_TILE - 1) / SSF_TILE);
    };
    int tx, tiles = tiles_of(H, W, tx);
    hipLaunchKernelGGL(ssf_blur_kernel<0>, dim3(planes * tiles), dim3(256), 0, st, x, hw, volume + hw, vps, H, W, tx,
                       tiles, taps);
    const float* prev = volume + hw;      // b_1 lives in the volume
    int64_t prev_ps = vps;
    for (int l = 2; l <= levels; ++l) {
        const int h = H >> (l - 1), w = W >> (l - 1);
        float* b = bbuf[l & 1];
        tiles = tiles_of(h, w, tx);
        hipLaunchKernelGGL(ssf_blur_kernel<1>, dim3(planes * tiles), dim3(256), 0, st, prev, prev_ps, b, (int64_t)h * w,
                           h, w, tx, tiles, taps);
        const float* s = b;
        for (int u = 1; u <= l - 1; ++u) {
            const int hi = h << (u - 1), wi = w << (u - 1);
            const bool last = u == l - 1;
            float* d = last ? volume + (int64_t)l * hw : ubuf[u & 1];
            hipLaunchKernelGGL(ssf_up2_kernel, dim3(ssf_grid((int64_t)planes * hi * wi * 4)), dim3(256), 0, st, s, d,
                               last ? vps : (int64_t)hi * wi * 4, (int64_t)planes, hi, wi);
            s = d;
        }
        prev = b;
        prev_ps = (int64_t)h * w;
    }
    CAI_LAUNCH_CHECK("ssf_volume_fwd");
    return CAI_OK;
}

int cai_ssf_volume_bwd(const float* dvolume, int32_t planes, int32_t H, int32_t W, float sigma, int32_t levels,
                       float* dx, void* workspace, size_t ws_bytes, void* stream) {
    int rc = ssf_check_shape("ssf_volume_bwd", planes, H, W, levels);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(dvolume && dx && workspace, "ssf_volume_bwd: null pointer");
    ssf_taps taps;
    const int K = ssf_make_taps(sigma, &taps);
    CAI_CHECK_ARG(K >= 1 && K <= SSF_MAX_TAPS, "ssf_volume_bwd: sigma %g gives %d taps (1..%d supported)", (double)sigma,
                  K, SSF_MAX_TAPS);
    if (ws_bytes < cai_ssf_workspace_bytes(planes, H, W, levels)) {
        set_error("ssf_volume_bwd: workspace of %zu bytes is too small", ws_bytes);
        return CAI_EWORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    const int64_t hw = (int64_t)H * W, vps = (int64_t)(levels + 1) * hw, q = (int64_t)planes * hw / 4;
    float* ws = (float*)workspace;
    float* db = ws;                          // db_l, up to [planes][H][W]
    float* dp = ws + 4 * q;                  // blur^T db_l, at most a quarter plane set
    float* ubuf[2] = {ws + 5 * q, ws + 6 * q};
    auto tiles_of = [](int h, int w, int& tx) {
        tx = (w + SSF_TILE - 1) / SSF_TILE;
        return tx * ((h + SSF_TILE - 1) / SSF_TILE);
    };
    const float* pool = nullptr;             // blur^T db_{l+1}, to be spread over level l's 2x2 cells
    for (int l = levels; l >= 1; --l) {
        const int h = H >> (l - 1), w = W >> (l - 1);
        // db_l = (up^T)^(l-1) dvol_l + pool^T(pool)
        const float* s = dvolume + (int64_t)l * hw;
        int64_t s_ps = vps;
        if (l == 1) {
            hipLaunchKernelGGL(ssf_up2t_kernel<0>, dim3(ssf_grid((int64_t)planes * h * w)), dim3(256), 0, st, s, s_ps,
                               pool, db, (int64_t)planes, h, w);
        }
        for (int u = l - 1; u >= 1; --u) {
            const int hi = h << (u - 1), wi = w << (u - 1);
            const bool last = u == 1;
            float* d = last ? db : ubuf[u & 1];
            hipLaunchKernelGGL(ssf_up2t_kernel<1>, dim3(ssf_grid((int64_t)planes * hi * wi)), dim3(256), 0, st, s, s_ps,
                               last ? pool : (const float*)nullptr, d, (int64_t)planes, hi, wi);
            s = d;
            s_ps = (int64_t)hi * wi;
        }
        int tx;
        const int tiles = tiles_of(h, w, tx);
        if (l == 1)
            hipLaunchKernelGGL(ssf_blurt_kernel, dim3(planes * tiles), dim3(256), 0, st, (const float*)db, dvolume, vps,
                               dx, h, w, tx, tiles, taps);
        else
            hipLaunchKernelGGL(ssf_blurt_kernel, dim3(planes * tiles), dim3(256), 0, st, (const float*)db,
                               (const float*)nullptr, (int64_t)0, dp, h, w, tx, tiles, taps);
        pool = dp;
    }
    CAI_LAUNCH_CHECK("ssf_volume_bwd");
    return CAI_OK;
}

static int ssf_warp_check(const char* what, const float* volume, const float* motion, const int64_t* ms, int32_t N,
                          int32_t C, int32_t D, int32_t H, int32_t W, ssf_warp_args* a) {
    CAI_CHECK_ARG(volume && motion && ms, "%s: null pointer", what);
    CAI_CHECK_ARG(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape [%d, %d, %d, %d, %d]", what, N, C, D, H,
                  W);
    CAI_CHECK_ARG((int64_t)N * C * D * H * W < (1ll << 40), "%s: volume too large", what);
    CAI_CHECK_ARG(ms[0] >= 0 && ms[1] >= 0 && ms[2] >= 0 && ms[3] >= 0, "%s: negative motion strides", what);
    a->vol = volume;
    a->motion = motion;
    a->m_sn = ms[0], a->m_sc = ms[1], a->m_sh = ms[2], a->m_sw = ms[3];
    a->N = N, a->C = C, a->D = D, a->H = H, a->W = W;
    return CAI_OK;
}

int cai_ssf_warp_fwd(const float* volume, const float* motion, const int64_t* motion_strides, int32_t N, int32_t C,
                     int32_t D, int32_t H, int32_t W, float* x_pred, const float* x_cur, float* x_res, void* stream) {
    ssf_warp_args a;
    int rc = ssf_warp_check("ssf_warp_fwd", volume, motion, motion_strides, N, C, D, H, W, &a);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(x_pred, "ssf_warp_fwd: null output");
    CAI_CHECK_ARG((x_cur == nullptr) == (x_res == nullptr), "ssf_warp_fwd: x_cur and x_res go together");
    hipLaunchKernelGGL(ssf_warp_fwd_kernel, dim3(ssf_grid((int64_t)N * H * W)), dim3(256), 0, as_stream(stream), a,
                       x_pred, x_cur, x_res);
    CAI_LAUNCH_CHECK("ssf_warp_fwd");
    return CAI_OK;
}

int cai_ssf_warp_bwd(const float* volume, const float* motion, const int64_t* motion_strides, int32_t N, int32_t C,
                     int32_t D, int32_t H, int32_t W, const float* g_pred, const float* g_res, float* d_motion,
                     float* d_volume, void* stream) {
    ssf_warp_args a;
    int rc = ssf_warp_check("ssf_warp_bwd", volume, motion, motion_strides, N, C, D, H, W, &a);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(g_pred || g_res, "ssf_warp_bwd: null upstream gradients");
    CAI_CHECK_ARG(d_motion || d_volume, "ssf_warp_bwd: null outputs");
    hipStream_t st = as_stream(stream);
    const int grid = ssf_grid((int64_t)N * H * W);
    if (d_motion)
        hipLaunchKernelGGL(ssf_warp_bwd_kernel<0>, dim3(grid), dim3(256), 0, st, a, g_pred, g_res, d_motion,
                           (float*)nullptr);
    if (d_volume)
        hipLaunchKernelGGL(ssf_warp_bwd_kernel<1>, dim3(grid), dim3(256), 0, st, a, g_pred, g_res, (float*)nullptr,
                           d_volume);
    CAI_LAUNCH_CHECK("ssf_warp_bwd");
    return CAI_OK;
}

}  // extern "C"
