// Fused autoregressive entropy coding of the context models (google.py:565-608, 654-692 of the reference):
// the whole raster scan of one image in one workgroup of one launch, no host round trip per latent pixel.
//
// Per pixel, in raster order: gather the 12 causal taps of the masked 5x5 context conv from y_hat, run the
// conv (M -> Cx) and the three 1x1 entropy-parameter layers (C0 = Cp + Cx -> C1 -> C2 -> 2M) as fp32
// matrix-vector products streamed from packed weights, split the result into scales / means, build the CDF
// indexes (GaussianConditional.build_indexes), then
//   encode: symbol = rintf(y - mean) (entropy.hip's symbols mode), written with its index for the host coder;
//   decode: the symbol comes from the rANS stream (rans_decode.hpp, the host coder's own state machine; the
//           CDF slot search is done by one wave instead of a binary search);
// and y_hat = float(symbol) + mean goes back to memory for the pixels to come.
//
// Workgroup b owns image b and never waits for another workgroup.  Both modes go through one device function
// for the parameters (ar_pixel_params): same weights, same fixed summation order, no atomics, so the
// decoder's y_hat is bit-identical to the encoder's, and independent of the batch size.  The params half of
// the first 1x1 layer does not depend on the scan; ar_hoist_kernel computes it for every pixel beforehand.
#include <algorithm>

#include "common.hpp"
#include "rans_decode.hpp"

namespace cai {

constexpr int AR_NT = 1024;          // threads of a scan workgroup (16 waves: one CU's worth)
constexpr int AR_TAPS = 12;          // causal taps of the 5x5 mask "A": rows -2, -1 full, row 0 its two left
constexpr int AR_MAX_SCALES = 256;   // scale-table cap
constexpr int AR_HOIST_NT = 256;
constexpr int AR_HOIST_PIX = 8;      // pixels per hoist block
constexpr size_t AR_MAX_LDS = 64 * 1024;

static inline int pad4(int n) { return (n + 3) & ~3; }

struct ar_lds_plan {
    int xin, h0, h1, h2, g, part, tab, idx, sym, total;   // float offsets
};

static ar_lds_plan ar_plan(const cai_ar_args* a) {
    ar_lds_plan p;
    int o = 0;
    p.xin = o; o += pad4(AR_TAPS * a->M);
    p.h0 = o; o += pad4(a->Cx);
    p.h1 = o; o += pad4(a->C1);
    p.h2 = o; o += pad4(a->C2);
    p.g = o; o += pad4(2 * a->M);
    p.part = o; o += 4 * AR_NT;
    p.tab = o; o += pad4(a->n_scales);
    p.idx = o; o += pad4(a->M);
    p.sym = o; o += pad4(a->M);
    p.total = o;
    return p;
}

struct ar_kargs {
    cai_ar_args a;
    ar_lds_plan p;
    const float* p1;   // hoisted first-layer half [B*H*W][C1] (bias included)
};

// out[o] = act(sum_k wt[k][o] x[k] + add[o]), o < O.  wt is [K][Opad] (Opad = pad4(O), zero columns past O).
// A thread owns four consecutive outputs of one K slice (16-byte coalesced weight reads, x broadcast from
// LDS); the slices' partial sums meet in LDS and are added in slice order.  x, part, out in LDS; add global.
__device__ __forceinline__ void ar_matvec(const float* __restrict__ wt, int K, int O, const float* x,
                                          const float* __restrict__ add, bool leaky, float slope, float* part,
                                          float* out) {
    const int tid = threadIdx.x;
    const int Opad = (O + 3) & ~3, O4 = Opad >> 2;
    const int ns = AR_NT / O4;
    const int kper = (K + ns - 1) / ns;
    const int sl = tid / O4, oq = tid - sl * O4;
    if (sl < ns) {
        const int k0 = sl * kper, k1 = min(K, k0 + kper);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const f32x4* wp = reinterpret_cast<const f32x4*>(wt) + (int64_t)k0 * O4 + oq;
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const f32x4 w0 = wp[0], w1 = wp[O4], w2 = wp[2 * O4], w3 = wp[3 * O4];
            const float x0 = x[k], x1 = x[k + 1], x2 = x[k + 2], x3 = x[k + 3];
            acc += w0 * x0;
            acc += w1 * x1;
            acc += w2 * x2;
            acc += w3 * x3;
            wp += 4 * O4;
        }
        for (; k < k1; ++k) {
            acc += wp[0] * x[k];
            wp += O4;
        }
        reinterpret_cast<f32x4*>(part)[sl * O4 + oq] = acc;
    }
    __syncthreads();
    for (int o = tid; o < O; o += AR_NT) {
        float s = part[o];
        for (int j = 1; j < ns; ++j) s += part[j * Opad + o];
        s += add[o];
        if (leaky) s = s > 0.f ? s : s * slope;
        out[o] = s;
    }
    __syncthreads();
}

// Entropy parameters of pixel (h, w) of image `img` (pixel offset of the image) from the y_hat written so far:
// leaves scales in g[0..M), means in g[M..2M) (LDS).  The one place both modes compute them.
__device__ __forceinline__ void ar_pixel_params(const ar_kargs& k, float* sm, int64_t img, int h, int w) {
    const cai_ar_args& a = k.a;
    const int M = a.M, W = a.W;
    float* xin = sm + k.p.xin;
    for (int i = threadIdx.x; i < AR_TAPS * M; i += AR_NT) {
        const int tap = i / M, c = i - tap * M;
        const int dy = tap < 5 ? -2 : (tap < 10 ? -1 : 0);
        const int dx = (tap < 10 ? tap % 5 : tap - 10) - 2;
        const int yy = h + dy, xx = w + dx;
        float v = 0.f;
        if (yy >= 0 && xx >= 0 && xx < W) v = a.y_hat[(img + (int64_t)yy * W + xx) * M + c];
        xin[i] = v;
    }
    __syncthreads();
    float* part = sm + k.p.part;
    ar_matvec(a.w_ctx, AR_TAPS * M, a.Cx, xin, a.b_ctx, false, 0.f, part, sm + k.p.h0);
    ar_matvec(a.w1c, a.Cx, a.C1, sm + k.p.h0, k.p1 + (img + (int64_t)h * W + w) * a.C1, true, a.slope, part,
              sm + k.p.h1);
    ar_matvec(a.w2, a.C1, a.C2, sm + k.p.h1, a.b2, true, a.slope, part, sm + k.p.h2);
    ar_matvec(a.w3, a.C2, 2 * M, sm + k.p.h2, a.b3, false, 0.f, part, sm + k.p.g);
}

// GaussianConditional.build_indexes: clamp at the bound, then L-1 - #{s in table[:-1] : scale <= s}
__device__ __forceinline__ int ar_index(float scale, float bound, const float* tab, int L) {
    return gc_scale_index(scale, bound, tab, L);
}

// The slot search of rans_decode.hpp's decode_symbol by a whole wave (every lane calls it with the same
// arguments and gets the same answer): the number of entries <= cum of the non-decreasing table, found by
// 64-way splits, minus one.  Reads stay inside cdf[0, size) whatever the table holds.
struct WaveSearch {
    __device__ int32_t operator()(const int32_t* cdf, int32_t size, uint32_t cum) const {
        const int lane = threadIdx.x & 63;
        int32_t lo = 0, n = size;
        while (n > 64) {   // <= 6 rounds
            const int32_t step = (n + 63) >> 6;
            const int32_t last = lo + min((lane + 1) * step, n) - 1;   // last entry of the lane's segment
            const int nfull = __popcll(__ballot(cdf[last] <= (int32_t)cum));
            if (nfull == 64) return lo + n - 1;
            const int32_t nlo = lo + nfull * step;
            n = min(step, lo + n - nlo);
            lo = nlo;
        }
        const bool le = lane < n && cdf[lo + lane] <= (int32_t)cum;
        return lo + __popcll(__ballot(le)) - 1;
    }
};

template <bool DECODE>
__global__ __launch_bounds__(AR_NT) void ar_scan_kernel(ar_kargs k) {
    extern __shared__ float sm[];
    __shared__ int s_status;
    const cai_ar_args& a = k.a;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = a.M, H = a.H, W = a.W, L = a.n_scales;
    const int64_t npix = (int64_t)H * W, img = (int64_t)b * npix;
    float* tab = sm + k.p.tab;
    float* g = sm + k.p.g;
    int* idx_s = reinterpret_cast<int*>(sm + k.p.idx);
    int* sym_s = reinterpret_cast<int*>(sm + k.p.sym);
    for (int i = tid; i < L; i += AR_NT) tab[i] = a.scale_table[i];

    cai_rans::DecState d;
    if (DECODE) {
        // every thread takes the same decision from the same values
        const int64_t off = a.offsets[b], len = a.lengths[b];
        bool ok = off >= 0 && len >= 8 && (off & 3) == 0 && (len & 3) == 0 && off <= a.data_bytes &&
                  len <= a.data_bytes - off;
        if (ok) ok = cai_rans::dec_init(d, reinterpret_cast<const uint32_t*>(a.data + off), len >> 2);
        if (!ok) {
            if (tid == 0) a.status[b] = cai_rans::kBadLength;
            return;
        }
    }
    __syncthreads();

    for (int64_t pix = 0; pix < npix; ++pix) {
        const int h = (int)(pix / W), w = (int)(pix - (int64_t)h * W);
        ar_pixel_params(k, sm, img, h, w);
        const int64_t e0 = (img + pix) * M;
        if (!DECODE) {
            for (int c = tid; c < M; c += AR_NT) {
                const float scale = g[c], mean = g[M + c];
                const int sym = (int)rintf(a.y[e0 + c] - mean);
                a.symbols[e0 + c] = sym;
                a.indexes[e0 + c] = ar_index(scale, a.scale_bound, tab, L);
                a.y_hat[e0 + c] = (float)sym + mean;
                if (a.scales) a.scales[e0 + c] = scale;
                if (a.means) a.means[e0 + c] = mean;
            }
        } else {
            for (int c = tid; c < M; c += AR_NT) idx_s[c] = ar_index(g[c], a.scale_bound, tab, L);
            __syncthreads();
            if (tid < 64) {   // wave 0 walks the stream; its lanes move in step and hold the same state
                int st = cai_rans::kOk;
                for (int c = 0; c < M; ++c) {
                    int32_t v = 0;
                    st = cai_rans::decode_symbol(d, idx_s[c], a.cdfs, (int64_t)a.cdf_stride, a.cdf_sizes,
                                                 a.cdf_offsets, a.n_cdfs, &v, WaveSearch());
                    if (st != cai_rans::kOk) break;
                    if (tid == 0) sym_s[c] = v;
                }
                if (tid == 0) s_status = st;
            }
            __syncthreads();
            const int st = s_status;
            if (st != cai_rans::kOk) {   // the stream stops here; nothing more of it is read
                if (tid == 0) a.status[b] = st;
                return;
            }
            for (int c = tid; c < M; c += AR_NT) {
                const float scale = g[c], mean = g[M + c];
                const int sym = sym_s[c];
                a.y_hat[e0 + c] = (float)sym + mean;
                if (a.symbols) a.symbols[e0 + c] = sym;
                if (a.indexes) a.indexes[e0 + c] = idx_s[c];
                if (a.scales) a.scales[e0 + c] = scale;
                if (a.means) a.means[e0 + c] = mean;
            }
        }
        __syncthreads();   // this pixel's y_hat is visible to the workgroup's next gathers
    }
    if (tid == 0 && a.status) a.status[b] = cai_rans::kOk;
}

// p1[pixel][o] = b1[o] + sum_k w1p[k][o] params[pixel][k]: the first 1x1 layer's params half, every pixel at
// once (AR_HOIST_PIX pixels per block, one weight read for all of them, k in order: no dependence on the grid)
__global__ __launch_bounds__(AR_HOIST_NT) void ar_hoist_kernel(const float* __restrict__ params,
                                                               const float* __restrict__ w1p,
                                                               const float* __restrict__ b1, float* __restrict__ p1,
                                                               int64_t npix, int Cp, int C1) {
    extern __shared__ float xs[];   // [AR_HOIST_PIX][Cp]
    const int64_t p0 = (int64_t)blockIdx.x * AR_HOIST_PIX;
    const int np = (int)min((int64_t)AR_HOIST_PIX, npix - p0);
    for (int i = threadIdx.x; i < AR_HOIST_PIX * Cp; i += AR_HOIST_NT) {
        const int p = i / Cp;
        xs[i] = p < np ? params[p0 * Cp + i] : 0.f;
    }
    __syncthreads();
    const int C1pad = (C1 + 3) & ~3;
    for (int o = threadIdx.x; o < C1; o += AR_HOIST_NT) {
        float acc[AR_HOIST_PIX];
        const float bias = b1[o];
#pragma unroll
        for (int p = 0; p < AR_HOIST_PIX; ++p) acc[p] = bias;
        for (int kk = 0; kk < Cp; ++kk) {
            const float wv = w1p[(int64_t)kk * C1pad + o];
#pragma unroll
            for (int p = 0; p < AR_HOIST_PIX; ++p) acc[p] = fmaf(wv, xs[p * Cp + kk], acc[p]);
        }
#pragma unroll
        for (int p = 0; p < AR_HOIST_PIX; ++p)
            if (p < np) p1[(p0 + p) * C1 + o] = acc[p];
    }
}

static int ar_check(const char* who, const cai_ar_args* a, bool decode, const void* workspace, size_t ws_bytes) {
    CAI_CHECK_ARG(a, "%s: null args", who);
    CAI_CHECK_ARG(a->B > 0 && a->H > 0 && a->W > 0 && a->M > 0, "%s: bad latent shape B=%d H=%d W=%d M=%d", who,
                  a->B, a->H, a->W, a->M);
    CAI_CHECK_ARG(a->Cp > 0 && a->Cx > 0 && a->C1 > 0 && a->C2 > 0, "%s: bad layer widths Cp=%d Cx=%d C1=%d C2=%d",
                  who, a->Cp, a->Cx, a->C1, a->C2);
    CAI_CHECK_ARG((int64_t)a->B * a->H * a->W * std::max(std::max(a->M, a->Cp), a->C1) < (int64_t)1 << 40 &&
                      (int64_t)a->H * a->W < (int64_t)1 << 31 && a->B <= 65535,
                  "%s: latent too large", who);
    const int widest = std::max(std::max(a->Cx, a->C1), std::max(a->C2, 2 * a->M));
    CAI_CHECK_ARG(pad4(widest) / 4 <= AR_NT, "%s: layer width %d exceeds %d", who, widest, 4 * AR_NT);
    CAI_CHECK_ARG(a->n_scales >= 1 && a->n_scales <= AR_MAX_SCALES, "%s: scale table of %d entries (1..%d supported)",
                  who, a->n_scales, AR_MAX_SCALES);
    CAI_CHECK_ARG((size_t)ar_plan(a).total * sizeof(float) <= AR_MAX_LDS &&
                      (size_t)AR_HOIST_PIX * a->Cp * sizeof(float) <= AR_MAX_LDS,
                  "%s: widths M=%d Cp=%d Cx=%d C1=%d C2=%d need more than %zu bytes of LDS", who, a->M, a->Cp, a->Cx,
                  a->C1, a->C2, AR_MAX_LDS);
    CAI_CHECK_ARG(a->params && a->w_ctx && a->b_ctx && a->w1p && a->w1c && a->b1 && a->w2 && a->b2 && a->w3 && a->b3 &&
                      a->scale_table && a->y_hat,
                  "%s: null pointer", who);
    for (const float* w : {a->w_ctx, a->w1p, a->w1c, a->w2, a->w3})
        CAI_CHECK_ARG((reinterpret_cast<uintptr_t>(w) & 15) == 0, "%s: packed weights must be 16-byte aligned", who);
    CAI_CHECK_ARG(a->slope == a->slope && a->scale_bound > 0.f, "%s: bad slope / scale bound", who);
    if (decode) {
        CAI_CHECK_ARG(a->data && a->offsets && a->lengths && a->status, "%s: null stream pointer", who);
        CAI_CHECK_ARG(a->data_bytes >= 0 && (reinterpret_cast<uintptr_t>(a->data) & 3) == 0,
                      "%s: the stream buffer must be 4-byte aligned", who);
        CAI_CHECK_ARG(a->cdfs && a->cdf_sizes && a->cdf_offsets && a->n_cdfs > 0 && a->cdf_stride >= 2,
                      "%s: invalid CDF tables", who);
        CAI_CHECK_ARG(a->n_scales <= a->n_cdfs, "%s: %d scales but %d CDFs", who, a->n_scales, a->n_cdfs);
    } else {
        CAI_CHECK_ARG(a->y && a->symbols && a->indexes, "%s: null pointer", who);
    }
    const size_t need = cai_ar_workspace_bytes(a);
    if (!workspace || ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, need %zu", who, workspace ? ws_bytes : (size_t)0, need);
        return CAI_EWORKSPACE;
    }
    return CAI_OK;
}

template <bool DECODE>
static int ar_run(const char* who, const cai_ar_args* a, void* workspace, size_t ws_bytes, void* stream) {
    const int rc = ar_check(who, a, DECODE, workspace, ws_bytes);
    if (rc) return rc;
    hipStream_t st = as_stream(stream);
    const int64_t npix = (int64_t)a->B * a->H * a->W;
    float* p1 = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(ar_hoist_kernel, dim3((unsigned)((npix + AR_HOIST_PIX - 1) / AR_HOIST_PIX)), dim3(AR_HOIST_NT),
                       (size_t)AR_HOIST_PIX * a->Cp * sizeof(float), st, a->params, a->w1p, a->b1, p1, npix, a->Cp,
                       a->C1);
    ar_kargs k;
    k.a = *a;
    k.p = ar_plan(a);
    k.p1 = p1;
    hipLaunchKernelGGL(ar_scan_kernel<DECODE>, dim3(a->B), dim3(AR_NT), (size_t)k.p.total * sizeof(float), st, k);
    CAI_LAUNCH_CHECK(who);
    return CAI_OK;
}

}  // namespace cai

using namespace cai;

extern "C" {

size_t cai_ar_workspace_bytes(const cai_ar_args* a) {
    if (!a || a->B <= 0 || a->H <= 0 || a->W <= 0 || a->C1 <= 0) {
        set_error("ar_workspace_bytes: bad shape");
        return 0;
    }
    return (size_t)a->B * a->H * a->W * a->C1 * sizeof(float);
}

int cai_ar_encode(const cai_ar_args* a, void* workspace, size_t ws_bytes, void* stream) {
    return ar_run<false>("ar_encode", a, workspace, ws_bytes, stream);
}

int cai_ar_decode(const cai_ar_args* a, void* workspace, size_t ws_bytes, void* stream) {
    return ar_run<true>("ar_decode", a, workspace, ws_bytes, stream);
}

}  // extern "C"
