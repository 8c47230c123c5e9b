// The per-frame path around the video codec when it is evaluated on raw YUV 4:2:0 (utils/video/eval_model): two
// launches per frame, fp32 arithmetic, integer planes in, exact integer error sums out; and, when it decodes to a raw
// file (utils/codec_rgbt), one launch per frame from the reconstruction to integer planes.
//
// yuv420 -> rgb    integer planar Y [H][W], U, V [H/2][W/2] (uint8 at 8 bits, uint16 above) -> fp32 planar RGB
//                  [3][Hp][Wp], the frame at (top, left) and zero around it: the model input.  Every sample is
//                  normalised by a true division c / max_val; the chroma planes are brought to H x W by a x2
//                  upsampling with align_corners = false semantics (nearest, bilinear or bicubic A = -0.75, whose
//                  weights at scale 2 are the two dyadic tap sets below; tap indices clamp to the plane); BT.709
//                  YCbCr -> RGB.  One thread owns one 2 x 2 luma quad: the chroma window is loaded once, filtered
//                  along W, then along H.  The cells tile the padded image from the frame's origin outwards, so
//                  the border is written by the same launch.  Optional second output org_q [3][H][W] =
//                  rint(clamp(rgb max_val, 0, max_val)), the levels the RGB metrics compare against.
// frame sse        reconstruction [3][Hp][Wp] at the same offsets -> rec_q [3][H][W] = rint(clamp(rec max_val, 0,
//                  max_val)) and four sums of squared level differences: Y, U, V (BT.709 RGB -> YCbCr of the
//                  clamped reconstruction, 2 x 2 mean of the chroma, rounded to levels, against the integer planes)
//                  and RGB (rec_q against org_q).  The differences are integers, so they are summed as integers:
//                  per thread, per wave, per block, then one 64-bit atomic add per block and sum.  Integer
//                  addition is order-free: the sums are bit-reproducible with no fixed-order reduce.
// rgb -> yuv420    reconstruction [3][Hp][Wp] at the same offsets -> the integer frame in file order, Y [H][W] then U
//                  and V [H/2][W/2] in one buffer (uint8 at 8 bits, uint16 above): the decoder's output, one copy and
//                  one write away from a .yuv file.  The levels come from the device function the frame sse measures
//                  (vid_quad_levels), so a written file has exactly the PSNR that was reported.  One thread per quad,
//                  plain vector stores, nothing shared.
#include <algorithm>

#include "common.hpp"

namespace cai {

constexpr double VID_KR_D = 0.2126, VID_KB_D = 0.0722;
constexpr float VID_KR = 0.2126f, VID_KG = 0.7152f, VID_KB = 0.0722f;
// the scalars the conversions multiply and divide by, formed in double and rounded once
constexpr float VID_R_CR = (float)(2.0 - 2.0 * VID_KR_D), VID_B_CB = (float)(2.0 - 2.0 * VID_KB_D);
constexpr float VID_1_KR = (float)(1.0 - VID_KR_D), VID_1_KB = (float)(1.0 - VID_KB_D);
// bicubic A = -0.75 at t = 3/4: output 2k reads k - 2 .. k + 1 with these, output 2k + 1 reads k - 1 .. k + 2 mirrored
constexpr float VID_C0 = -0.03515625f, VID_C1 = 0.26171875f, VID_C2 = 0.87890625f, VID_C3 = -0.10546875f;

enum { VID_NEAREST = 0, VID_BILINEAR = 1, VID_BICUBIC = 2 };

template <int MODE> struct vid_radius { static constexpr int value = MODE == VID_BICUBIC ? 2 : MODE == VID_BILINEAR ? 1 : 0; };

// the two outputs 2k (even) and 2k + 1 (odd) of one axis from the window t[0 .. 2R] centred on sample k
template <int MODE>
__device__ __forceinline__ void vid_up2(const float (&t)[2 * vid_radius<MODE>::value + 1], bool first, float& even,
                                        float& odd) {
    if (MODE == VID_BICUBIC) {
        even = VID_C0 * t[0] + VID_C1 * t[1] + VID_C2 * t[2] + VID_C3 * t[3];
        odd = VID_C3 * t[1] + VID_C2 * t[2] + VID_C1 * t[3] + VID_C0 * t[4];
    } else if (MODE == VID_BILINEAR) {
        // output 0 sits at source coordinate -1/4, which is clamped to 0: sample 0 itself
        even = first ? t[1] : 0.25f * t[0] + 0.75f * t[1];
        odd = 0.75f * t[1] + 0.25f * t[2];
    } else {
        even = odd = t[0];
    }
}

// plane [h][w] of T around (ky, kx), normalised and upsampled to the quad's four positions: o[0] o[1] / o[2] o[3]
template <int MODE, typename T>
__device__ __forceinline__ void vid_chroma_quad(const T* __restrict__ p, int h, int w, int ky, int kx, float mv,
                                                float (&o)[4]) {
    constexpr int R = vid_radius<MODE>::value, N = 2 * R + 1;
    float ev[N], od[N];
#pragma unroll
    for (int dy = 0; dy < N; ++dy) {
        const int y = min(max(ky + dy - R, 0), h - 1);
        float t[N];
#pragma unroll
        for (int dx = 0; dx < N; ++dx) {
            const int x = min(max(kx + dx - R, 0), w - 1);
            t[dx] = (float)p[(int64_t)y * w + x] / mv;
        }
        vid_up2<MODE>(t, kx == 0, ev[dy], od[dy]);
    }
    vid_up2<MODE>(ev, ky == 0, o[0], o[2]);
    vid_up2<MODE>(od, ky == 0, o[1], o[3]);
}

__device__ __forceinline__ float vid_level(float v, float mv) { return rintf(fminf(fmaxf(v * mv, 0.f), mv)); }

__device__ __forceinline__ float vid_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// One 2 x 2 quad of the clamped reconstruction, c[channel][pixel], as 4:2:0 levels: BT.709 RGB -> YCbCr, the four Y
// and the quad's mean Cb and Cr, rounded.  The frame-sse kernel measures these levels and the writer stores them:
// one body, so what is written is what was measured.  The luma sum KR r + KG g + KB b is the one expression here
// that the compiler may contract, and how it does so depends on the code around the call (the writer got a packed
// multiply and a plain add where the frame-sse kernel has two fused steps): the fused steps are therefore spelled
// out, in the form the frame-sse kernel has always been compiled to -- the rounded green product first.
__device__ __forceinline__ void vid_quad_levels(const float (&c)[3][4], float mv, float (&yq)[4], float& uq,
                                                float& vq) {
    float cbs = 0.f, crs = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float y = fmaf(VID_KB, c[2][k], fmaf(VID_KR, c[0][k], VID_KG * c[1][k]));
        cbs += 0.5f * (c[2][k] - y) / VID_1_KB + 0.5f;
        crs += 0.5f * (c[0][k] - y) / VID_1_KR + 0.5f;
        yq[k] = vid_level(y, mv);
    }
    uq = vid_level(cbs * 0.25f, mv);
    vq = vid_level(crs * 0.25f, mv);
}

struct vid_geom {
    int32_t H, W, Hp, Wp, top, left;
    int32_t cy0, cx0, ncy, ncx;   // cells (2 x 2, origin at the frame's corner) that cover the padded image
};

// VEC: left and Wp even and the images 8-byte aligned, so a cell's row is one aligned float2
template <int MODE, typename T, int VEC>
__global__ __launch_bounds__(256) void yuv420_to_rgb_kernel(const T* __restrict__ Y, const T* __restrict__ U,
                                                            const T* __restrict__ V, const vid_geom g, float mv,
                                                            float* __restrict__ rgb, float* __restrict__ org_q) {
    const int64_t cells = (int64_t)g.ncy * g.ncx;
    const int64_t ps = (int64_t)g.Hp * g.Wp, fs = (int64_t)g.H * g.W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t)gridDim.x * 256) {
        const int cy = (int)(i / g.ncx) + g.cy0, cx = (int)(i % g.ncx) + g.cx0;
        const int fy = 2 * cy, fx = 2 * cx;            // frame coordinates of the cell's corner
        const int py = g.top + fy, px = g.left + fx;   // and in the padded image
        float c[3][4];
        const bool inside = fy >= 0 && fy < g.H && fx >= 0 && fx < g.W;
        if (inside) {
            float yy[4], cb[4], cr[4];
            const T* yr = Y + (int64_t)fy * g.W + fx;
            yy[0] = (float)yr[0] / mv;
            yy[1] = (float)yr[1] / mv;
            yy[2] = (float)yr[g.W] / mv;
            yy[3] = (float)yr[g.W + 1] / mv;
            vid_chroma_quad<MODE>(U, g.H >> 1, g.W >> 1, cy, cx, mv, cb);
            vid_chroma_quad<MODE>(V, g.H >> 1, g.W >> 1, cy, cx, mv, cr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float r = yy[k] + VID_R_CR * (cr[k] - 0.5f);
                const float b = yy[k] + VID_B_CB * (cb[k] - 0.5f);
                c[0][k] = r;
                c[1][k] = (yy[k] - VID_KR * r - VID_KB * b) / VID_KG;
                c[2][k] = b;
            }
            if (org_q) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float* q = org_q + ch * fs + (int64_t)fy * g.W + fx;
                    if (VEC) {
                        *reinterpret_cast<float2*>(q) = make_float2(vid_level(c[ch][0], mv), vid_level(c[ch][1], mv));
                        *reinterpret_cast<float2*>(q + g.W) =
                            make_float2(vid_level(c[ch][2], mv), vid_level(c[ch][3], mv));
                    } else {
                        q[0] = vid_level(c[ch][0], mv);
                        q[1] = vid_level(c[ch][1], mv);
                        q[g.W] = vid_level(c[ch][2], mv);
                        q[g.W + 1] = vid_level(c[ch][3], mv);
                    }
                }
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int k = 0; k < 4; ++k) c[ch][k] = 0.f;
        }
        // a border cell may hang over the padded image's edge: rows and columns are clipped one by one
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = py + r;
            if (y < 0 || y >= g.Hp) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float* d = rgb + ch * ps + (int64_t)y * g.Wp;
                if (VEC) {   // px is even: both columns are in or both are out
                    if (px >= 0 && px < g.Wp)
                        *reinterpret_cast<float2*>(d + px) = make_float2(c[ch][2 * r], c[ch][2 * r + 1]);
                } else {
                    if (px >= 0 && px < g.Wp) d[px] = c[ch][2 * r];
                    if (px + 1 >= 0 && px + 1 < g.Wp) d[px + 1] = c[ch][2 * r + 1];
                }
            }
        }
    }
}

__device__ __forceinline__ unsigned long long vid_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ unsigned long long vid_sq(float a, float b) {
    const int d = (int)a - (int)b;                  // levels are integers below 2^16
    const unsigned ad = (unsigned)(d < 0 ? -d : d);
    return (unsigned long long)(ad * ad);           // < 2^32
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void video_frame_sse_kernel(const T* __restrict__ Y, const T* __restrict__ U,
                                                              const T* __restrict__ V, const vid_geom g, float mv,
                                                              const float* __restrict__ org_q,
                                                              const float* __restrict__ rec,
                                                              float* __restrict__ rec_q,
                                                              unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[4][4];
    const int hw2 = g.W >> 1;
    const int64_t quads = (int64_t)(g.H >> 1) * hw2;
    const int64_t ps = (int64_t)g.Hp * g.Wp, fs = (int64_t)g.H * g.W;
    unsigned long long acc[4] = {0, 0, 0, 0};      // Y, U, V, RGB
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const int ky = (int)(i / hw2), kx = (int)(i % hw2);
        const int fy = 2 * ky, fx = 2 * kx;
        float c[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = rec + ch * ps + (int64_t)(g.top + fy) * g.Wp + g.left + fx;
            const float* o = org_q + ch * fs + (int64_t)fy * g.W + fx;
            float oq[4];
            if (VEC) {
                const float2 a = *reinterpret_cast<const float2*>(s), b = *reinterpret_cast<const float2*>(s + g.Wp);
                const float2 oa = *reinterpret_cast<const float2*>(o), ob = *reinterpret_cast<const float2*>(o + g.W);
                c[ch][0] = a.x, c[ch][1] = a.y, c[ch][2] = b.x, c[ch][3] = b.y;
                oq[0] = oa.x, oq[1] = oa.y, oq[2] = ob.x, oq[3] = ob.y;
            } else {
                c[ch][0] = s[0], c[ch][1] = s[1], c[ch][2] = s[g.Wp], c[ch][3] = s[g.Wp + 1];
                oq[0] = o[0], oq[1] = o[1], oq[2] = o[g.W], oq[3] = o[g.W + 1];
            }
            float q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[ch][k] = vid_clamp01(c[ch][k]);
                q[k] = vid_level(c[ch][k], mv);
                acc[3] += vid_sq(q[k], oq[k]);
            }
            if (rec_q) {
                float* d = rec_q + ch * fs + (int64_t)fy * g.W + fx;
                if (VEC) {
                    *reinterpret_cast<float2*>(d) = make_float2(q[0], q[1]);
                    *reinterpret_cast<float2*>(d + g.W) = make_float2(q[2], q[3]);
                } else {
                    d[0] = q[0], d[1] = q[1], d[g.W] = q[2], d[g.W + 1] = q[3];
                }
            }
        }
        const T* yr = Y + (int64_t)fy * g.W + fx;
        const float yo[4] = {(float)yr[0], (float)yr[1], (float)yr[g.W], (float)yr[g.W + 1]};
        float yq[4], uq, vq;
        vid_quad_levels(c, mv, yq, uq, vq);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0] += vid_sq(yq[k], yo[k]);
        acc[1] += vid_sq(uq, (float)U[(int64_t)ky * hw2 + kx]);
        acc[2] += vid_sq(vq, (float)V[(int64_t)ky * hw2 + kx]);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long s = vid_wave_sum(acc[k]);
        if (lane == 0) part[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long s =
            (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (s) atomicAdd(sums + threadIdx.x, s);
    }
}

template <typename T> struct alignas(2 * sizeof(T)) vid_pair { T a, b; };

// VEC & 1: left and Wp even and rec 8-byte aligned, so a quad's row is one aligned float2.  VEC & 2: out aligned to
// two samples, so the two Y levels of a row (W and fx are even) are one aligned two-sample store.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void rgb_to_yuv420_kernel(const float* __restrict__ rec, const vid_geom g, float mv,
                                                            T* __restrict__ out) {
    const int hw2 = g.W >> 1;
    const int64_t quads = (int64_t)(g.H >> 1) * hw2;
    const int64_t ps = (int64_t)g.Hp * g.Wp, fs = (int64_t)g.H * g.W;
    T* U = out + fs;      // file order: Y [H][W], U [H/2][W/2], V
    T* V = U + quads;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const int ky = (int)(i / hw2), kx = (int)(i % hw2);
        const int fy = 2 * ky, fx = 2 * kx;
        float c[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = rec + ch * ps + (int64_t)(g.top + fy) * g.Wp + g.left + fx;
            if (VEC & 1) {
                const float2 a = *reinterpret_cast<const float2*>(s), b = *reinterpret_cast<const float2*>(s + g.Wp);
                c[ch][0] = a.x, c[ch][1] = a.y, c[ch][2] = b.x, c[ch][3] = b.y;
            } else {
                c[ch][0] = s[0], c[ch][1] = s[1], c[ch][2] = s[g.Wp], c[ch][3] = s[g.Wp + 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) c[ch][k] = vid_clamp01(c[ch][k]);
        }
        float yq[4], uq, vq;
        vid_quad_levels(c, mv, yq, uq, vq);
        T* d = out + (int64_t)fy * g.W + fx;     // levels are integers in [0, 65535]
        if (VEC & 2) {
            *reinterpret_cast<vid_pair<T>*>(d) = vid_pair<T>{(T)(int)yq[0], (T)(int)yq[1]};
            *reinterpret_cast<vid_pair<T>*>(d + g.W) = vid_pair<T>{(T)(int)yq[2], (T)(int)yq[3]};
        } else {
            d[0] = (T)(int)yq[0], d[1] = (T)(int)yq[1], d[g.W] = (T)(int)yq[2], d[g.W + 1] = (T)(int)yq[3];
        }
        U[i] = (T)(int)uq;
        V[i] = (T)(int)vq;
    }
}

static int vid_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(16384, (n + 255) / 256)); }

static bool vid_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

static int vid_check(const char* what, const void* y, const void* u, const void* v, int32_t H, int32_t W,
                     int32_t bitdepth, int32_t Hp, int32_t Wp, int32_t top, int32_t left, vid_geom* g) {
    CAI_CHECK_ARG(y && u && v, "%s: null plane", what);
    CAI_CHECK_ARG(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: H = %d and W = %d must be even and >= 2 (4:2:0)",
                  what, H, W);
    CAI_CHECK_ARG(bitdepth == 8 || bitdepth == 10 || bitdepth == 12 || bitdepth == 14 || bitdepth == 16,
                  "%s: bit depth %d not in {8, 10, 12, 14, 16}", what, bitdepth);
    CAI_CHECK_ARG(top >= 0 && left >= 0, "%s: negative padding (top %d, left %d)", what, top, left);
    CAI_CHECK_ARG(Hp >= 1 && Wp >= 1 && (int64_t)top + H <= Hp && (int64_t)left + W <= Wp,
                  "%s: the %d x %d frame at (%d, %d) does not fit the padded %d x %d image", what, H, W, top, left, Hp,
                  Wp);
    CAI_CHECK_ARG((int64_t)Hp * Wp < (1ll << 30), "%s: image too large", what);
    if (bitdepth > 8)
        CAI_CHECK_ARG(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) &
                       1) == 0,
                      "%s: 16-bit planes must be 2-byte aligned", what);
    g->H = H, g->W = W, g->Hp = Hp, g->Wp = Wp, g->top = top, g->left = left;
    g->cy0 = -((top + 1) / 2);
    g->cx0 = -((left + 1) / 2);
    g->ncy = (Hp - top + 1) / 2 - g->cy0;
    g->ncx = (Wp - left + 1) / 2 - g->cx0;
    return CAI_OK;
}

template <int MODE, typename T>
static void launch_to_rgb(bool vec, int grid, hipStream_t st, const void* y, const void* u, const void* v,
                          const vid_geom& g, float mv, float* rgb, float* org_q) {
    if (vec)
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<MODE, T, 1>), dim3(grid), dim3(256), 0, st, (const T*)y, (const T*)u,
                           (const T*)v, g, mv, rgb, org_q);
    else
        hipLaunchKernelGGL((yuv420_to_rgb_kernel<MODE, T, 0>), dim3(grid), dim3(256), 0, st, (const T*)y, (const T*)u,
                           (const T*)v, g, mv, rgb, org_q);
}

template <typename T>
static void launch_to_rgb_mode(int mode, bool vec, int grid, hipStream_t st, const void* y, const void* u,
                               const void* v, const vid_geom& g, float mv, float* rgb, float* org_q) {
    if (mode == VID_BICUBIC)
        launch_to_rgb<VID_BICUBIC, T>(vec, grid, st, y, u, v, g, mv, rgb, org_q);
    else if (mode == VID_BILINEAR)
        launch_to_rgb<VID_BILINEAR, T>(vec, grid, st, y, u, v, g, mv, rgb, org_q);
    else
        launch_to_rgb<VID_NEAREST, T>(vec, grid, st, y, u, v, g, mv, rgb, org_q);
}

}  // namespace cai

using namespace cai;

extern "C" {

int cai_yuv420_to_rgb(const void* y, const void* u, const void* v, int32_t H, int32_t W, int32_t bitdepth,
                      int32_t mode, float* rgb, int32_t Hp, int32_t Wp, int32_t top, int32_t left, float* org_q,
                      void* stream) {
    vid_geom g;
    int rc = vid_check("yuv420_to_rgb", y, u, v, H, W, bitdepth, Hp, Wp, top, left, &g);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(mode == VID_NEAREST || mode == VID_BILINEAR || mode == VID_BICUBIC,
                  "yuv420_to_rgb: unknown upsampling mode %d (0 nearest, 1 bilinear, 2 bicubic)", mode);
    CAI_CHECK_ARG(rgb, "yuv420_to_rgb: null output");
    const bool vec = left % 2 == 0 && Wp % 2 == 0 && vid_aligned8(rgb) && vid_aligned8(org_q);
    const float mv = (float)((1 << bitdepth) - 1);
    const int grid = vid_grid((int64_t)g.ncy * g.ncx);
    hipStream_t st = as_stream(stream);
    if (bitdepth == 8)
        launch_to_rgb_mode<uint8_t>(mode, vec, grid, st, y, u, v, g, mv, rgb, org_q);
    else
        launch_to_rgb_mode<uint16_t>(mode, vec, grid, st, y, u, v, g, mv, rgb, org_q);
    CAI_LAUNCH_CHECK("yuv420_to_rgb");
    return CAI_OK;
}

int cai_video_frame_sse(const void* y, const void* u, const void* v, int32_t H, int32_t W, int32_t bitdepth,
                        const float* org_q, const float* rec, int32_t Hp, int32_t Wp, int32_t top, int32_t left,
                        uint64_t* sums, float* rec_q, void* stream) {
    vid_geom g;
    int rc = vid_check("video_frame_sse", y, u, v, H, W, bitdepth, Hp, Wp, top, left, &g);
    if (rc != CAI_OK) return rc;
    CAI_CHECK_ARG(org_q && rec && sums, "video_frame_sse: null pointer");
    CAI_CHECK_ARG(vid_aligned8(sums), "video_frame_sse: the sums must be 8-byte aligned");
    const bool vec = left % 2 == 0 && Wp % 2 == 0 && vid_aligned8(rec) && vid_aligned8(org_q) && vid_aligned8(rec_q);
    const float mv = (float)((1 << bitdepth) - 1);
    const int grid = vid_grid((int64_t)(H / 2) * (W / 2));
    hipStream_t st = as_stream(stream);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
#define CAI_SSE_LAUNCH(T, VEC)                                                                                     \
    hipLaunchKernelGGL((video_frame_sse_kernel<T, VEC>), dim3(grid), dim3(256), 0, st, (const T*)y, (const T*)u,    \
                       (const T*)v, g, mv, org_q, rec, rec_q, out)
    if (bitdepth == 8) {
        if (vec) CAI_SSE_LAUNCH(uint8_t, 1); else CAI_SSE_LAUNCH(uint8_t, 0);
    } else {
        if (vec) CAI_SSE_LAUNCH(uint16_t, 1); else CAI_SSE_LAUNCH(uint16_t, 0);
    }
#undef CAI_SSE_LAUNCH
    CAI_LAUNCH_CHECK("video_frame_sse");
    return CAI_OK;
}

int cai_rgb_to_yuv420(const float* rec, int32_t Hp, int32_t Wp, int32_t top, int32_t left, int32_t H, int32_t W,
                      int32_t bitdepth, void* out, void* stream) {
    CAI_CHECK_ARG(rec && out, "rgb_to_yuv420: null pointer");
    vid_geom g;
    int rc = vid_check("rgb_to_yuv420", out, out, out, H, W, bitdepth, Hp, Wp, top, left, &g);   // the planes are out's
    if (rc != CAI_OK) return rc;
    const int sample = bitdepth == 8 ? 1 : 2;
    const int vec = (left % 2 == 0 && Wp % 2 == 0 && vid_aligned8(rec) ? 1 : 0) |
                    ((reinterpret_cast<uintptr_t>(out) & (uintptr_t)(2 * sample - 1)) == 0 ? 2 : 0);
    const float mv = (float)((1 << bitdepth) - 1);
    const int grid = vid_grid((int64_t)(H / 2) * (W / 2));
    hipStream_t st = as_stream(stream);
#define CAI_YUV_LAUNCH(T, VEC)                                                                                     \
    hipLaunchKernelGGL((rgb_to_yuv420_kernel<T, VEC>), dim3(grid), dim3(256), 0, st, rec, g, mv, (T*)out)
#define CAI_YUV_LAUNCH_T(T)                                                                                        \
    switch (vec) {                                                                                                 \
        case 3: CAI_YUV_LAUNCH(T, 3); break;                                                                       \
        case 2: CAI_YUV_LAUNCH(T, 2); break;                                                                       \
        case 1: CAI_YUV_LAUNCH(T, 1); break;                                                                       \
        default: CAI_YUV_LAUNCH(T, 0); break;                                                                      \
    }
    if (bitdepth == 8) {
        CAI_YUV_LAUNCH_T(uint8_t)
    } else {
        CAI_YUV_LAUNCH_T(uint16_t)
    }
#undef CAI_YUV_LAUNCH_T
#undef CAI_YUV_LAUNCH
    CAI_LAUNCH_CHECK("rgb_to_yuv420");
    return CAI_OK;
}

}  // extern "C"
