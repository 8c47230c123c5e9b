// The coding front end and back end of the entropy models: everything between a pixel-major latent and the host
// coder's integer arrays, one launch each way.
//
//   code_front ... x, (scales, means) or per-channel means -> symbols and indexes in the coder's order, x_hat
//   code_back .... decoded symbols in the coder's order, means -> x_hat
//
// The latent is pixel-major, element (p, c) of image b at ptr[(b P + p) ld + c] with P = H W; the coder's order is
// NCHW, element (p, c) at [(b C + c) P + p] (what symbols.reshape(B, -1) yields for a [B, C, H, W] tensor).  The
// work is that transpose.  A block owns a tile of 64 pixels x 64 channels of one image and stages it through LDS:
// the float accesses run along the channels and the integer accesses along the pixels, so both sides coalesce.
//
// Tile shape and banks.  The tile is stored [channel][pixel] with a pitch of 65 dwords, so (channel, pixel) sits on
// bank (channel + pixel) mod 32 for the 4-byte LDS accesses used here.  On the 16-byte path thread t takes the
// quad t & 7 of the contiguous axis and the row t >> 3 of the other: a 32-lane group is 8 quads x 4 rows, element e
// of quad q in row r lands on bank (4 q + e + r + const) mod 32 -- 32 distinct banks for every e, on the channel
// side and on the pixel side alike -- and eight lanes cover 128 contiguous bytes of global memory.  Four such
// 32 x 32 passes fill or drain the tile.  On the scalar path a 32-lane group walks 32 consecutive channels (or
// pixels) of one row: 32 distinct banks again.  The LDS reads stay 4 bytes wide: the odd pitch leaves no 16-byte
// alignment, and a misaligned ds_read_b128 costs more than the four reads.
//
// Each side picks its width on its own: 16-byte float accesses need C, every ld and the float pointers to allow
// them, 16-byte integer accesses need P % 4 == 0 and aligned integer pointers.  Partial tiles occur on both axes;
// with 16-byte accesses a quad is either inside or outside (C, respectively P, is a multiple of 4 there).
//
// The integers are those of the composed ops: gc_round / gc_scale_index (common.hpp) as in cai_quantize, the fused
// autoregressive scan and the checkerboard passes.  x_hat on the per-element path is rint(x - mean) + mean, the
// float form cai_quantize's DEQUANTIZE mode writes; on the per-channel path and in code_back it is
// float(symbol) + mean, EntropyModel.dequantize's form.  No atomics, no allocation, no scratch.
#include "common.hpp"

namespace cai {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int CF_TP = 64;            // pixels per tile
constexpr int CF_TC = 64;            // channels per tile
constexpr int CF_PITCH = CF_TP + 1;  // dwords between the tile's channel rows
constexpr int CF_NT = 256;

struct CodeTile {
    int b, p0, c0;
};

// block -> (image, pixel tile, channel tile); the channel tiles of a pixel tile are adjacent blocks
__device__ __forceinline__ CodeTile code_tile(int P, int C) {
    const int tc = (C + CF_TC - 1) / CF_TC, tp = (P + CF_TP - 1) / CF_TP;
    const int blk = blockIdx.x;
    const int ic = blk % tc, rest = blk / tc;
    CodeTile t;
    t.b = rest / tp;
    t.p0 = (rest - t.b * tp) * CF_TP;
    t.c0 = ic * CF_TC;
    return t;
}

struct CodeFrontArgs {
    const float* x;        // null: indexes only
    const float* scales;   // null: per-channel mode (means [C], index = channel)
    const float* means;
    const float* tab;
    int L;
    float bound;
    float* x_hat;
    int* symbols;
    int* indexes;
    int x_ld, s_ld, m_ld, xh_ld;
    int P, C;
};

// VF: 16-byte accesses on the float (channel-contiguous) side; VI: on the integer (pixel-contiguous) side
template <bool VF, bool VI>
__global__ __launch_bounds__(CF_NT) void code_front_kernel(const CodeFrontArgs a) {
    __shared__ int s_sym[CF_TC * CF_PITCH];
    __shared__ int s_idx[CF_TC * CF_PITCH];
    const CodeTile T = code_tile(a.P, a.C);
    const int t = threadIdx.x;
    const int64_t pix0 = (int64_t)T.b * a.P;
    const bool per_channel = a.scales == nullptr;

    if (VF) {
        const int q = t & 7, r = t >> 3;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int cl = (pass & 1) * 32 + q * 4, pl = (pass >> 1) * 32 + r;
            const int c = T.c0 + cl, p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t pix = pix0 + p;
            f32x4 mu = {0.f, 0.f, 0.f, 0.f};
            i32x4 idx;
            if (per_channel) {
                mu = *reinterpret_cast<const f32x4*>(a.means + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) idx[e] = c + e;
            } else {
                const f32x4 s = *reinterpret_cast<const f32x4*>(a.scales + pix * a.s_ld + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) idx[e] = gc_scale_index(s[e], a.bound, a.tab, a.L);
                if (a.x) mu = *reinterpret_cast<const f32x4*>(a.means + pix * a.m_ld + c);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) s_idx[(cl + e) * CF_PITCH + pl] = idx[e];
            if (a.x) {   // the same for every thread
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + pix * a.x_ld + c);
                f32x4 xh;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float rr = gc_round(v[e], mu[e]);
                    const int sym = (int)rr;
                    s_sym[(cl + e) * CF_PITCH + pl] = sym;
                    xh[e] = per_channel ? (float)sym + mu[e] : rr + mu[e];
                }
                *reinterpret_cast<f32x4*>(a.x_hat + pix * a.xh_ld + c) = xh;
            }
        }
    } else {
        const int cl = t & 63, c = T.c0 + cl;
        for (int pl = t >> 6; pl < CF_TP; pl += CF_NT / 64) {
            const int p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t pix = pix0 + p;
            float mu = 0.f;
            int idx;
            if (per_channel) {
                mu = a.means[c];
                idx = c;
            } else {
                idx = gc_scale_index(a.scales[pix * a.s_ld + c], a.bound, a.tab, a.L);
                if (a.x) mu = a.means[pix * a.m_ld + c];
            }
            s_idx[cl * CF_PITCH + pl] = idx;
            if (a.x) {
                const float rr = gc_round(a.x[pix * a.x_ld + c], mu);
                const int sym = (int)rr;
                s_sym[cl * CF_PITCH + pl] = sym;
                a.x_hat[pix * a.xh_ld + c] = per_channel ? (float)sym + mu : rr + mu;
            }
        }
    }
    __syncthreads();

    const int64_t plane0 = (int64_t)T.b * a.C;
    if (VI) {
        const int q = t & 7, r = t >> 3;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int pl = (pass & 1) * 32 + q * 4, cl = (pass >> 1) * 32 + r;
            const int c = T.c0 + cl, p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t o = (plane0 + c) * a.P + p;
            i32x4 idx;
#pragma unroll
            for (int e = 0; e < 4; ++e) idx[e] = s_idx[cl * CF_PITCH + pl + e];
            *reinterpret_cast<i32x4*>(a.indexes + o) = idx;
            if (a.x) {
                i32x4 sym;
#pragma unroll
                for (int e = 0; e < 4; ++e) sym[e] = s_sym[cl * CF_PITCH + pl + e];
                *reinterpret_cast<i32x4*>(a.symbols + o) = sym;
            }
        }
    } else {
        const int pl = t & 63, p = T.p0 + pl;
        for (int cl = t >> 6; cl < CF_TC; cl += CF_NT / 64) {
            const int c = T.c0 + cl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t o = (plane0 + c) * a.P + p;
            a.indexes[o] = s_idx[cl * CF_PITCH + pl];
            if (a.x) a.symbols[o] = s_sym[cl * CF_PITCH + pl];
        }
    }
}

struct CodeBackArgs {
    const int* symbols;
    const float* means;
    float* x_hat;
    int m_ld, xh_ld;   // m_ld 0: per-channel means [C]
    int P, C;
};

template <bool VF, bool VI>
__global__ __launch_bounds__(CF_NT) void code_back_kernel(const CodeBackArgs a) {
    __shared__ int s_sym[CF_TC * CF_PITCH];
    const CodeTile T = code_tile(a.P, a.C);
    const int t = threadIdx.x;
    const int64_t plane0 = (int64_t)T.b * a.C;

    if (VI) {
        const int q = t & 7, r = t >> 3;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int pl = (pass & 1) * 32 + q * 4, cl = (pass >> 1) * 32 + r;
            const int c = T.c0 + cl, p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const i32x4 sym = *reinterpret_cast<const i32x4*>(a.symbols + (plane0 + c) * a.P + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) s_sym[cl * CF_PITCH + pl + e] = sym[e];
        }
    } else {
        const int pl = t & 63, p = T.p0 + pl;
        for (int cl = t >> 6; cl < CF_TC; cl += CF_NT / 64) {
            const int c = T.c0 + cl;
            if (c >= a.C || p >= a.P) continue;
            s_sym[cl * CF_PITCH + pl] = a.symbols[(plane0 + c) * a.P + p];
        }
    }
    __syncthreads();

    const int64_t pix0 = (int64_t)T.b * a.P;
    const bool per_channel = a.m_ld == 0;
    if (VF) {
        const int q = t & 7, r = t >> 3;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int cl = (pass & 1) * 32 + q * 4, pl = (pass >> 1) * 32 + r;
            const int c = T.c0 + cl, p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t pix = pix0 + p;
            const f32x4 mu = *reinterpret_cast<const f32x4*>(per_channel ? a.means + c : a.means + pix * a.m_ld + c);
            f32x4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = (float)s_sym[(cl + e) * CF_PITCH + pl] + mu[e];
            *reinterpret_cast<f32x4*>(a.x_hat + pix * a.xh_ld + c) = xh;
        }
    } else {
        const int cl = t & 63, c = T.c0 + cl;
        for (int pl = t >> 6; pl < CF_TP; pl += CF_NT / 64) {
            const int p = T.p0 + pl;
            if (c >= a.C || p >= a.P) continue;
            const int64_t pix = pix0 + p;
            const float mu = per_channel ? a.means[c] : a.means[pix * a.m_ld + c];
            a.x_hat[pix * a.xh_ld + c] = (float)s_sym[cl * CF_PITCH + pl] + mu;
        }
    }
}

static inline bool cf_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int code_shape(const char* what, int32_t B, int32_t H, int32_t W, int32_t C, int* P, int64_t* blocks) {
    CAI_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1, "%s: bad shape B %d H %d W %d C %d", what, B, H, W, C);
    CAI_CHECK_ARG((int64_t)B * H * W * C < (1ll << 31), "%s: B H W C must be below 2^31", what);
    *P = H * W;
    *blocks = (int64_t)B * ((*P + CF_TP - 1) / CF_TP) * ((C + CF_TC - 1) / CF_TC);   // <= B H W C: below 2^31
    return CAI_OK;
}

}  // namespace cai

using namespace cai;

#define CODE_LAUNCH(kernel, vf, vi, blocks, st, a)                                                          \
    do {                                                                                                    \
        const dim3 g_((unsigned)(blocks)), b_(CF_NT);                                                       \
        if ((vf) && (vi))                                                                                   \
            hipLaunchKernelGGL((kernel<true, true>), g_, b_, 0, st, a);                                     \
        else if (vf)                                                                                        \
            hipLaunchKernelGGL((kernel<true, false>), g_, b_, 0, st, a);                                    \
        else if (vi)                                                                                        \
            hipLaunchKernelGGL((kernel<false, true>), g_, b_, 0, st, a);                                    \
        else                                                                                                \
            hipLaunchKernelGGL((kernel<false, false>), g_, b_, 0, st, a);                                   \
    } while (0)

extern "C" {

int cai_code_front(const float* x, int32_t x_ld, const float* scales, int32_t s_ld, const float* means,
                   int32_t m_ld, const float* scale_table, int32_t n_scales, float scale_bound, int32_t B, int32_t H,
                   int32_t W, int32_t C, float* x_hat, int32_t xh_ld, int32_t* symbols, int32_t* indexes,
                   void* stream) {
    const char* what = x ? "code_front" : "code_indexes";
    CodeFrontArgs a{};
    int64_t blocks;
    const int rc = code_shape(what, B, H, W, C, &a.P, &blocks);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(indexes, "%s: null pointer", what);
    CAI_CHECK_ARG(x || scales, "%s: null pointer (neither a latent nor scales)", what);
    bool vf = C % 4 == 0;
    if (scales) {
        CAI_CHECK_ARG(scale_table, "%s: null pointer", what);
        CAI_CHECK_ARG(n_scales >= 1 && s_ld >= C, "%s: bad scale table or scales pitch", what);
        vf = vf && s_ld % 4 == 0 && cf_al16(scales);
    }
    if (x) {
        CAI_CHECK_ARG(means && x_hat && symbols, "%s: null pointer", what);
        CAI_CHECK_ARG(x_ld >= C && xh_ld >= C && (!scales || m_ld >= C), "%s: row pitch below the row width", what);
        vf = vf && x_ld % 4 == 0 && xh_ld % 4 == 0 && (!scales || m_ld % 4 == 0) && cf_al16(x) && cf_al16(means) &&
             cf_al16(x_hat);
    }
    const bool vi = a.P % 4 == 0 && cf_al16(indexes) && (!x || cf_al16(symbols));
    a.x = x; a.scales = scales; a.means = means; a.tab = scale_table; a.L = n_scales; a.bound = scale_bound;
    a.x_hat = x_hat; a.symbols = symbols; a.indexes = indexes;
    a.x_ld = x_ld; a.s_ld = s_ld; a.m_ld = m_ld; a.xh_ld = xh_ld;
    a.C = C;
    CODE_LAUNCH(code_front_kernel, vf, vi, blocks, as_stream(stream), a);
    CAI_LAUNCH_CHECK(what);
    return CAI_OK;
}

int cai_code_indexes(const float* scales, int32_t s_ld, const float* scale_table, int32_t n_scales, float scale_bound,
                     int32_t B, int32_t H, int32_t W, int32_t C, int32_t* indexes, void* stream) {
    CAI_CHECK_ARG(scales, "code_indexes: null pointer");
    return cai_code_front(nullptr, 0, scales, s_ld, nullptr, 0, scale_table, n_scales, scale_bound, B, H, W, C,
                          nullptr, 0, nullptr, indexes, stream);
}

int cai_code_back(const int32_t* symbols, const float* means, int32_t m_ld, int32_t B, int32_t H, int32_t W,
                  int32_t C, float* x_hat, int32_t xh_ld, void* stream) {
    CodeBackArgs a{};
    int64_t blocks;
    const int rc = code_shape("code_back", B, H, W, C, &a.P, &blocks);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(symbols && means && x_hat, "code_back: null pointer");
    CAI_CHECK_ARG((m_ld == 0 || m_ld >= C) && xh_ld >= C, "code_back: row pitch below the row width");
    const bool vf = C % 4 == 0 && m_ld % 4 == 0 && xh_ld % 4 == 0 && cf_al16(means) && cf_al16(x_hat);
    const bool vi = a.P % 4 == 0 && cf_al16(symbols);
    a.symbols = symbols; a.means = means; a.x_hat = x_hat;
    a.m_ld = m_ld; a.xh_ld = xh_ld;
    a.C = C;
    CODE_LAUNCH(code_back_kernel, vf, vi, blocks, as_stream(stream), a);
    CAI_LAUNCH_CHECK("code_back");
    return CAI_OK;
}

}  // extern "C"
