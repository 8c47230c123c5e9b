// Checkerboard context models (He et al., "Checkerboard Context Model for Efficient Learned Image Compression",
// CVPR 2021): the parity kernels around the two dense passes of compressai/models/google.py (_ARCoding).
//
// A position (h, w) is an anchor iff (h + w) is odd (parity 1).  The anchors are coded from the hyperprior alone,
// the non-anchors (parity 0) from the hyperprior and a masked conv over the decoded anchors.  The masked conv and
// the 1x1 entropy-parameter stack run over the whole map on the conv kernels; what is left per pass is elementwise
// work on the positions of one parity:
//   parity_zero ....... out = x with one parity zeroed (the context features at the anchors; its own backward)
//   ckbd_quantize ..... indexes / symbols of a parity into the coder's order, y_hat at the parity's positions
//   ckbd_dequantize ... the decoded integers of a parity + means -> y_hat at the parity's positions
//
// All tensors are pixel-major, element (p, c) at ptr[p * ld + c]; consecutive lanes walk the channels of a
// position, so loads and stores coalesce, 16 bytes per lane where C, the lds and the pointers allow it.  The coding
// kernels are launched over the parity's positions only: work item -> (image, slot, channel group), the position
// follows from the slot in closed form (ckbd_pos), so no lane is idle and no branch depends on the parity of a
// lane's position.  HBM-bound, no LDS.
//
// The coder's order of one image: the anchors' slots 0 .. n1 - 1, then the non-anchors' n1 .. H W - 1, each group
// in raster order.  Within its group position (h, w) has slot h (W / 2) + (w >> 1) for even W and (h W + w) >> 1 for
// odd W (there the parity of the linear index is the parity of h + w).
#include "common.hpp"

#include <algorithm>

namespace cai {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct CkbdMap {
    int H, W, C;
    int parity;
    int npar;    // positions of the parity per image
    int nbase;   // first slot of the parity's group: 0 (anchors), n1 (non-anchors)
    int half;    // W / 2 for even W, 0 for odd W
};

// (h, w) of slot k of the map's parity
__device__ __forceinline__ void ckbd_pos(const CkbdMap& m, int k, int& h, int& w) {
    if (m.half) {   // even W: every row holds W / 2 positions of either parity, the row's first at (h + parity) & 1
        h = k / m.half;
        w = 2 * (k - h * m.half) + ((h + m.parity) & 1);
    } else {        // odd W: the positions of the parity are the linear indexes of that parity
        const int i = 2 * k + m.parity;
        h = i / m.W;
        w = i - h * m.W;
    }
}

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float F; typedef int I; };
template <> struct VecOf<4> { typedef f32x4 F; typedef i32x4 I; };
__device__ __forceinline__ float lane_of(float v, int) { return v; }
__device__ __forceinline__ float lane_of(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ void set_lane(float& v, int, float s) { v = s; }
__device__ __forceinline__ void set_lane(f32x4& v, int e, float s) { v[e] = s; }
__device__ __forceinline__ int lane_of(int v, int) { return v; }
__device__ __forceinline__ int lane_of(const i32x4& v, int e) { return v[e]; }
__device__ __forceinline__ void set_lane(int& v, int, int s) { v = s; }
__device__ __forceinline__ void set_lane(i32x4& v, int e, int s) { v[e] = s; }

struct CkbdQuantArgs {
    CkbdMap m;
    int B;
    const float* y;        // null: indexes only
    const float* scales;
    const float* means;
    const float* tab;
    int L;
    float bound;
    float* y_hat;
    int* symbols;
    int* indexes;
    int y_ld, s_ld, m_ld, yh_ld;
};

template <int V>
__global__ __launch_bounds__(256) void ckbd_quantize_kernel(const CkbdQuantArgs a) {
    typedef typename VecOf<V>::F FV;
    typedef typename VecOf<V>::I IV;
    const CkbdMap m = a.m;
    const int CV = m.C / V;
    const int64_t HW = (int64_t)m.H * m.W;
    const int64_t n = (int64_t)a.B * m.npar * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = t / CV;
        const int c = (int)(t - q * CV) * V;
        const int b = (int)(q / m.npar), k = (int)(q - (int64_t)b * m.npar);
        int h, w;
        ckbd_pos(m, k, h, w);
        const int64_t p = b * HW + (int64_t)h * m.W + w;
        const int64_t slot = (b * HW + m.nbase + k) * m.C + c;
        const FV s = *reinterpret_cast<const FV*>(a.scales + p * a.s_ld + c);
        IV idx;
#pragma unroll
        for (int e = 0; e < V; ++e) set_lane(idx, e, gc_scale_index(lane_of(s, e), a.bound, a.tab, a.L));
        *reinterpret_cast<IV*>(a.indexes + slot) = idx;
        if (a.y) {   // the same for every thread
            const FV mu = *reinterpret_cast<const FV*>(a.means + p * a.m_ld + c);
            const FV v = *reinterpret_cast<const FV*>(a.y + p * a.y_ld + c);
            IV sym;
            FV q_hat;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float r = gc_round(lane_of(v, e), lane_of(mu, e));
                set_lane(sym, e, (int)r);
                set_lane(q_hat, e, (float)(int)r + lane_of(mu, e));
            }
            *reinterpret_cast<IV*>(a.symbols + slot) = sym;
            *reinterpret_cast<FV*>(a.y_hat + p * a.yh_ld + c) = q_hat;
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void ckbd_dequantize_kernel(const CkbdMap m, int B, const int* __restrict__ symbols,
                                                              const float* __restrict__ means, int m_ld,
                                                              float* __restrict__ y_hat, int yh_ld) {
    typedef typename VecOf<V>::F FV;
    typedef typename VecOf<V>::I IV;
    const int CV = m.C / V;
    const int64_t HW = (int64_t)m.H * m.W;
    const int64_t n = (int64_t)B * m.npar * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = t / CV;
        const int c = (int)(t - q * CV) * V;
        const int b = (int)(q / m.npar), k = (int)(q - (int64_t)b * m.npar);
        int h, w;
        ckbd_pos(m, k, h, w);
        const int64_t p = b * HW + (int64_t)h * m.W + w;
        const IV sym = *reinterpret_cast<const IV*>(symbols + (b * HW + m.nbase + k) * m.C + c);
        const FV mu = *reinterpret_cast<const FV*>(means + p * m_ld + c);
        FV out;
#pragma unroll
        for (int e = 0; e < V; ++e) set_lane(out, e, (float)lane_of(sym, e) + lane_of(mu, e));
        *reinterpret_cast<FV*>(y_hat + p * yh_ld + c) = out;
    }
}

// out = x with one parity zeroed, in units U of the row (16-byte groups, or single elements): every thread stores,
// the kept positions load first.  A wave spans a few positions of both parities; the select is a masked load.
template <typename U>
__global__ __launch_bounds__(256) void parity_zero_kernel(const U* __restrict__ x, int64_t x_ld, U* __restrict__ out,
                                                          int64_t out_ld, int64_t n, int CU, int H, int W, int parity) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = t / CU;
        const int cu = (int)(t - pix * CU);
        const int64_t row = pix / W;
        const int w = (int)(pix - row * W), h = (int)(row % H);
        U v = U();
        if (((h + w) & 1) != parity) v = x[pix * x_ld + cu];
        out[pix * out_ld + cu] = v;
    }
}

static inline int ckbd_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048)); }

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int ckbd_map(const char* what, int32_t B, int32_t H, int32_t W, int32_t C, int32_t parity, CkbdMap* m) {
    CAI_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: bad shape B %d H %d W %d C %d", what, B, H, W, C);
    CAI_CHECK_ARG((int64_t)B * H * W * C < (1ll << 31), "%s: B H W C must be below 2^31", what);
    CAI_CHECK_ARG(parity == 0 || parity == 1, "%s: parity %d is neither 0 nor 1", what, parity);
    const int64_t hw = (int64_t)H * W;
    const int n1 = (int)(hw / 2);
    m->H = H; m->W = W; m->C = C; m->parity = parity;
    m->npar = parity ? n1 : (int)(hw - n1);
    m->nbase = parity ? 0 : n1;
    m->half = (W & 1) ? 0 : W / 2;
    return CAI_OK;
}

}  // namespace cai

using namespace cai;

extern "C" {

int cai_parity_zero(int dtype, const void* x, int32_t x_ld, void* out, int32_t out_ld, int32_t B, int32_t H,
                    int32_t W, int32_t C, int32_t parity, void* stream) {
    CAI_CHECK_ARG(dtype == CAI_BF16 || dtype == CAI_F32, "parity_zero: bad dtype");
    CAI_CHECK_ARG(x && out && x != out, "parity_zero: null or aliased pointer");
    CkbdMap m;
    const int rc = ckbd_map("parity_zero", B, H, W, C, parity, &m);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(x_ld >= C && out_ld >= C, "parity_zero: row pitch below the row width");
    const int es = dtype_size(dtype);
    const int64_t npix = (int64_t)B * H * W;
    hipStream_t st = as_stream(stream);
    if ((int64_t)C * es % 16 == 0 && (int64_t)x_ld * es % 16 == 0 && (int64_t)out_ld * es % 16 == 0 && al16(x) &&
        al16(out)) {
        const int CU = C * es / 16;
        const int64_t n = npix * CU;
        hipLaunchKernelGGL(parity_zero_kernel<u32x4>, dim3(ckbd_grid(n)), dim3(256), 0, st, (const u32x4*)x,
                           (int64_t)x_ld * es / 16, (u32x4*)out, (int64_t)out_ld * es / 16, n, CU, H, W, parity);
    } else if (dtype == CAI_BF16) {
        const int64_t n = npix * C;
        hipLaunchKernelGGL(parity_zero_kernel<unsigned short>, dim3(ckbd_grid(n)), dim3(256), 0, st,
                           (const unsigned short*)x, (int64_t)x_ld, (unsigned short*)out, (int64_t)out_ld, n, C, H, W,
                           parity);
    } else {
        const int64_t n = npix * C;
        hipLaunchKernelGGL(parity_zero_kernel<unsigned>, dim3(ckbd_grid(n)), dim3(256), 0, st, (const unsigned*)x,
                           (int64_t)x_ld, (unsigned*)out, (int64_t)out_ld, n, C, H, W, parity);
    }
    CAI_LAUNCH_CHECK("parity_zero");
    return CAI_OK;
}

int cai_ckbd_quantize(const float* y, int32_t y_ld, const float* scales, int32_t s_ld, const float* means,
                      int32_t m_ld, const float* scale_table, int32_t n_scales, float scale_bound, int32_t B,
                      int32_t H, int32_t W, int32_t C, int32_t parity, float* y_hat, int32_t yh_ld, int32_t* symbols,
                      int32_t* indexes, void* stream) {
    const char* what = y ? "ckbd_quantize" : "ckbd_indexes";
    CkbdQuantArgs a{};
    const int rc = ckbd_map(what, B, H, W, C, parity, &a.m);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(scales && scale_table && indexes, "%s: null pointer", what);
    CAI_CHECK_ARG(n_scales >= 1 && s_ld >= C, "%s: bad scale table or scales pitch", what);
    bool vec = C % 4 == 0 && s_ld % 4 == 0 && al16(scales) && al16(indexes);
    if (y) {
        CAI_CHECK_ARG(means && y_hat && symbols, "%s: null pointer", what);
        CAI_CHECK_ARG(y_ld >= C && m_ld >= C && yh_ld >= C, "%s: row pitch below the row width", what);
        vec = vec && y_ld % 4 == 0 && m_ld % 4 == 0 && yh_ld % 4 == 0 && al16(y) && al16(means) && al16(y_hat) &&
              al16(symbols);
    }
    a.B = B;
    a.y = y; a.scales = scales; a.means = means; a.tab = scale_table; a.L = n_scales; a.bound = scale_bound;
    a.y_hat = y_hat; a.symbols = symbols; a.indexes = indexes;
    a.y_ld = y_ld; a.s_ld = s_ld; a.m_ld = m_ld; a.yh_ld = yh_ld;
    const int64_t n = (int64_t)B * a.m.npar * (vec ? C / 4 : C);
    if (n == 0) return CAI_OK;   // a 1 x 1 map has no anchors
    if (vec)
        hipLaunchKernelGGL(ckbd_quantize_kernel<4>, dim3(ckbd_grid(n)), dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(ckbd_quantize_kernel<1>, dim3(ckbd_grid(n)), dim3(256), 0, as_stream(stream), a);
    CAI_LAUNCH_CHECK(what);
    return CAI_OK;
}

int cai_ckbd_indexes(const float* scales, int32_t s_ld, const float* scale_table, int32_t n_scales, float scale_bound,
                     int32_t B, int32_t H, int32_t W, int32_t C, int32_t parity, int32_t* indexes, void* stream) {
    return cai_ckbd_quantize(nullptr, 0, scales, s_ld, nullptr, 0, scale_table, n_scales, scale_bound, B, H, W, C,
                             parity, nullptr, 0, nullptr, indexes, stream);
}

int cai_ckbd_dequantize(const int32_t* symbols, const float* means, int32_t m_ld, int32_t B, int32_t H, int32_t W,
                        int32_t C, int32_t parity, float* y_hat, int32_t yh_ld, void* stream) {
    CkbdMap m;
    const int rc = ckbd_map("ckbd_dequantize", B, H, W, C, parity, &m);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(symbols && means && y_hat, "ckbd_dequantize: null pointer");
    CAI_CHECK_ARG(m_ld >= C && yh_ld >= C, "ckbd_dequantize: row pitch below the row width");
    const bool vec = C % 4 == 0 && m_ld % 4 == 0 && yh_ld % 4 == 0 && al16(symbols) && al16(means) && al16(y_hat);
    const int64_t n = (int64_t)B * m.npar * (vec ? C / 4 : C);
    if (n == 0) return CAI_OK;
    if (vec)
        hipLaunchKernelGGL(ckbd_dequantize_kernel<4>, dim3(ckbd_grid(n)), dim3(256), 0, as_stream(stream), m, B,
                           symbols, means, m_ld, y_hat, yh_ld);
    else
        hipLaunchKernelGGL(ckbd_dequantize_kernel<1>, dim3(ckbd_grid(n)), dim3(256), 0, as_stream(stream), m, B,
                           symbols, means, m_ld, y_hat, yh_ld);
    CAI_LAUNCH_CHECK("ckbd_dequantize");
    return CAI_OK;
}

}  // extern "C"
