// Multi-scale SSIM (the pytorch_msssim definition restated in compressai/utils/metrics.py) as a training
// distortion and evaluation metric: 11-tap Gaussian window (sigma 1.5, separable, "valid"), K = (0.01, 0.03),
// five scales with 2x2 average pooling (padding side % 2, divisor 4) between them, ReLU on the per-plane scale
// means, product of powers per plane, mean over the planes.  fp32 throughout.
//
// forward   pool x 4 (the X / Y pyramids) -> msssim_fwd_kernel (every scale of every plane in one grid of
//           32x32 output tiles, a few consecutive tiles per block, one partial sum per tile; optionally the
//           backward's coefficient maps a, b, c) -> msssim_fold_kernel (one wave per plane: its partials in a
//           fixed order, the per-plane value) -> msssim_mean_kernel (one block).  No atomics: bit-reproducible.
// backward  one launch per scale from 4 down to 0: the adjoint of the same separable window over a, b, c
//           (zero outside the valid region), combined with X(p), Y(p), scaled by the plane's kappa_s, plus the
//           pooling chain 1/4 dX_{s+1}[(p + pad) / 2].
// Both tile kernels are bound by latency, not by arithmetic (41 / 37 KB of LDS: 3 / 4 blocks per CU), so a block
// loads its next tile into registers while it filters the current one.
//
// With m1, m2, m11, m22, m12 the windowed moments at output q, D1 = m1^2 + m2^2 + C1, D2 = s1 + s2 + C2:
//   cs = (2 s12 + C2) / D2,  l = (2 m1 m2 + C1) / D1
//   d cs(q) / d X(p) = g(p - q) [a + b X(p) + c Y(p)],  a = 2 (cs m1 - m2) / D2, b = -2 cs / D2, c = 2 / D2
//   d (l cs)(q) / d X(p): a' = cs 2 (m2 - l m1) / D1 + l a, b' = l b, c' = l c
#include <algorithm>

#include "common.hpp"

namespace cai {

constexpr int MS_SCALES = 5;
constexpr int MS_WIN = 11;
constexpr int MS_HALO = MS_WIN - 1;
constexpr int MS_TILE = 32;
constexpr int MS_IN = MS_TILE + MS_HALO;          // 42: rows / columns a tile's window reaches
constexpr int MS_MIN_SIDE = MS_HALO * 16;         // a side must exceed this for five scales
constexpr int MS_LD = (MS_IN * MS_IN + 255) / 256;   // registers per thread that hold one 42 x 42 plane of a tile
constexpr int MS_FWD_SLOTS = 256 * 3;             // forward blocks resident at once: 256 CUs x 3 (41 KB of LDS each)
constexpr int MS_BWD_SLOTS = 256 * 4;             // backward: 37 KB of LDS each

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, rounded from double
#define MS_G0 1.028380084e-03f
#define MS_G1 7.598758135e-03f
#define MS_G2 3.600077213e-02f
#define MS_G3 1.093606895e-01f
#define MS_G4 2.130055377e-01f
#define MS_G5 2.660117249e-01f
__device__ __forceinline__ constexpr float ms_g(int k) {
    return k == 0 || k == 10 ? MS_G0 : k == 1 || k == 9 ? MS_G1 : k == 2 || k == 8 ? MS_G2
         : k == 3 || k == 7 ? MS_G3 : k == 4 || k == 6 ? MS_G4 : MS_G5;
}
__host__ __device__ __forceinline__ constexpr float ms_weight(int s) {
    return s == 0 ? 0.0448f : s == 1 ? 0.2856f : s == 2 ? 0.3001f : s == 3 ? 0.2363f : 0.1333f;
}

// element s of a five-entry register array by a block-uniform index (selects, not an indexed copy)
template <typename T>
__device__ __forceinline__ T ms_pick(const T (&v)[MS_SCALES], int s) {
    return s == 0 ? v[0] : (s == 1 ? v[1] : (s == 2 ? v[2] : (s == 3 ? v[3] : v[4])));
}

struct ms_fwd_args {
    const float* x[MS_SCALES];     // [planes][H_s][W_s]
    const float* y[MS_SCALES];
    float* abc[MS_SCALES];         // a of scale s on the same grid (b at + abc_stride, c at + 2 abc_stride); null: not kept
    int64_t blk0[MS_SCALES];       // first tile of scale s in the forward grid
    int64_t abc_stride;
    int64_t total_tiles;
    int32_t tiles_per_block;
    int32_t H[MS_SCALES], W[MS_SCALES];
    int32_t tiles_x[MS_SCALES], tiles[MS_SCALES];   // output tiles per row / per plane
    float C1, C2;
};

struct ms_fold_args {
    int64_t blk0[MS_SCALES];
    int32_t tiles[MS_SCALES];
    float inv_n[MS_SCALES];        // 1 / valid outputs of a plane
};

struct ms_bwd_args {
    const float* x;                // this scale's planes
    const float* y;
    const float* abc;
    int64_t abc_stride;
    const float* vals;             // [planes][5] clamped scale means
    const float* per_plane;        // [planes] MS-SSIM of the plane
    const float* g_mean;           // upstream gradient of the mean (device scalar, nullable = 0)
    const float* g_plane;          // upstream gradients of the per-plane values (nullable = 0)
    const float* dnext;            // dX of the next (coarser) scale, null at the last
    float* dx;
    int32_t H, W, Hn, Wn;
    int64_t total_tiles;
    int32_t tiles_per_block;
    int32_t tiles_x, tiles;        // input tiles per row / per plane
    int32_t scale;
    float coef;                    // w_s / n_s
    float inv_planes;
};

// out[r][j] = sum_k g(k) in[r][j + k] for the NQ planes of a 42 x 42 tile -> 42 x 32
template <int NQ>
__device__ __forceinline__ void ms_hpass(const float (&raw)[NQ][MS_IN][MS_IN], float (&hp)[NQ][MS_IN][MS_TILE]) {
    for (int i = threadIdx.x; i < MS_IN * MS_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        float s[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n) s[n] = 0.f;
#pragma unroll
        for (int k = 0; k < MS_WIN; ++k)
#pragma unroll
            for (int n = 0; n < NQ; ++n) s[n] = fmaf(ms_g(k), raw[n][r][j + k], s[n]);
#pragma unroll
        for (int n = 0; n < NQ; ++n) hp[n][r][j] = s[n];
    }
}

// acc[n][o] = sum_k g(k) hp[n][row0 + o + k][col], o = 0..3
template <int NQ>
__device__ __forceinline__ void ms_vpass(const float (&hp)[NQ][MS_IN][MS_TILE], int row0, int col, float (&acc)[NQ][4]) {
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[n][o] = 0.f;
#pragma unroll
    for (int r = 0; r < MS_WIN + 3; ++r) {
        float v[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n) v[n] = hp[n][row0 + r][col];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = r - o;
            if (k >= 0 && k < MS_WIN) {
#pragma unroll
                for (int n = 0; n < NQ; ++n) acc[n][o] = fmaf(ms_g(k), v[n], acc[n][o]);
            }
        }
    }
}

// 2x2 average pooling of X and Y, padding (H % 2, W % 2) counted in the divisor: [planes][H][W] -> [planes][Hn][Wn]
__global__ __launch_bounds__(256) void msssim_pool_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          float* __restrict__ xo, float* __restrict__ yo,
                                                          int64_t planes, int H, int W, int Hn, int Wn) {
    const int64_t n = planes * Hn * Wn;
    const int ph = H & 1, pw = W & 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % Wn);
        const int64_t t = i / Wn;
        const int oy = (int)(t % Hn);
        const int64_t base = (t / Hn) * H * W;
        const int iy = 2 * oy - ph, ix = 2 * ox - pw;
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int yy = iy + dy, xx = ix + dx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    const int64_t j = base + (int64_t)yy * W + xx;
                    sx += x[j];
                    sy += y[j];
                }
            }
        xo[i] = 0.25f * sx;
        yo[i] = 0.25f * sy;
    }
}

// tile t of the forward grid: scale, plane and origin (block-uniform)
struct ms_fwd_tile {
    int s, H, W, q0y, q0x;
    int64_t plane;
};

// The per-scale entries are read from the kernel-argument segment by index (the struct is the kernel's first
// argument: offset 0): scalar loads of the one scale in use.  Selecting among the by-value copies kept all five
// scales' pointers and sizes in SGPRs across the tile loop and spilled them to VGPR lanes.
typedef const __attribute__((address_space(4))) ms_fwd_args* ms_fwd_kargs;
__device__ __forceinline__ ms_fwd_kargs ms_fwd_kernarg() {
    return (ms_fwd_kargs)__builtin_amdgcn_kernarg_segment_ptr();
}

__device__ __forceinline__ ms_fwd_tile ms_fwd_decode(const ms_fwd_args& a, int64_t t) {
    ms_fwd_tile c;
    c.s = 0;
#pragma unroll
    for (int i = 1; i < MS_SCALES; ++i)
        if (t >= a.blk0[i]) c.s = i;
    const ms_fwd_kargs k = ms_fwd_kernarg();
    c.H = k->H[c.s];
    c.W = k->W[c.s];
    const uint32_t tiles = (uint32_t)k->tiles[c.s], tiles_x = (uint32_t)k->tiles_x[c.s];
    const uint32_t lid = (uint32_t)(t - k->blk0[c.s]);   // the host keeps the whole grid below 2^31 tiles
    const uint32_t plane = lid / tiles, tile = lid - plane * tiles, ty = tile / tiles_x;
    c.plane = plane;
    c.q0y = (int)ty * MS_TILE;
    c.q0x = (int)(tile - ty * tiles_x) * MS_TILE;
    return c;
}

// the tile's 42 x 42 pixels of X and Y (zero past the plane), element threadIdx.x + 256 m in register m
__device__ __forceinline__ void ms_fwd_load(const ms_fwd_args& a, const ms_fwd_tile& c, float (&rx)[MS_LD],
                                            float (&ry)[MS_LD]) {
    const ms_fwd_kargs k = ms_fwd_kernarg();
    const float* __restrict__ X = k->x[c.s] + c.plane * c.H * c.W;
    const float* __restrict__ Y = k->y[c.s] + c.plane * c.H * c.W;
#pragma unroll
    for (int m = 0; m < MS_LD; ++m) {
        const int i = threadIdx.x + 256 * m;
        const int gy = c.q0y + i / MS_IN, gx = c.q0x + i % MS_IN;
        const bool ok = i < MS_IN * MS_IN && gy < c.H && gx < c.W;
        const int64_t j = (int64_t)gy * c.W + gx;
        rx[m] = ok ? X[j] : 0.f;
        ry[m] = ok ? Y[j] : 0.f;
    }
}

__global__ __launch_bounds__(256) void msssim_fwd_kernel(ms_fwd_args a, float* __restrict__ part) {
    __shared__ float raw[2][MS_IN][MS_IN];
    __shared__ float hp[5][MS_IN][MS_TILE];
    __shared__ float red[4];
    // a block walks tiles_per_block consecutive tiles; the next tile's pixels are loaded into registers while
    // this one is filtered (three blocks fit a CU: without it the load latency of every tile is exposed)
    const int64_t t_last = ((int64_t)blockIdx.x + 1) * a.tiles_per_block;
    const int64_t t_end = t_last < a.total_tiles ? t_last : a.total_tiles;
    ms_fwd_tile cur = ms_fwd_decode(a, (int64_t)blockIdx.x * a.tiles_per_block);
    float rx[MS_LD], ry[MS_LD];
    ms_fwd_load(a, cur, rx, ry);
  for (int64_t bid = (int64_t)blockIdx.x * a.tiles_per_block; bid < t_end; ++bid) {
    const int s = cur.s, H = cur.H, W = cur.W, q0y = cur.q0y, q0x = cur.q0x;
    const int64_t plane = cur.plane;
    float* __restrict__ A = ms_fwd_kernarg()->abc[s];
    const bool last = s == MS_SCALES - 1;
#pragma unroll
    for (int m = 0; m < MS_LD; ++m) {
        const int i = threadIdx.x + 256 * m;
        if (i < MS_IN * MS_IN) {
            (&raw[0][0][0])[i] = rx[m];
            (&raw[1][0][0])[i] = ry[m];
        }
    }
    __syncthreads();
    if (bid + 1 < t_end) {
        cur = ms_fwd_decode(a, bid + 1);
        ms_fwd_load(a, cur, rx, ry);
    }
    // horizontal pass over x, y, x^2, y^2, xy
    for (int i = threadIdx.x; i < MS_IN * MS_TILE; i += 256) {
        const int r = i >> 5, j = i & 31;
        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
        for (int k = 0; k < MS_WIN; ++k) {
            const float xv = raw[0][r][j + k], yv = raw[1][r][j + k], g = ms_g(k);
            sx = fmaf(g, xv, sx);
            sy = fmaf(g, yv, sy);
            sxx = fmaf(g, xv * xv, sxx);
            syy = fmaf(g, yv * yv, syy);
            sxy = fmaf(g, xv * yv, sxy);
        }
        hp[0][r][j] = sx;
        hp[1][r][j] = sy;
        hp[2][r][j] = sxx;
        hp[3][r][j] = syy;
        hp[4][r][j] = sxy;
    }
    __syncthreads();
    const int col = threadIdx.x & 31, row0 = (threadIdx.x >> 5) * 4;
    float acc[5][4];
    ms_vpass<5>(hp, row0, col, acc);

    const int OH = H - MS_HALO, OW = W - MS_HALO;
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int qy = q0y + row0 + o, qx = q0x + col;
        if (qy < OH && qx < OW) {
            const float m1 = acc[0][o], m2 = acc[1][o];
            const float s1 = fmaf(-m1, m1, acc[2][o]), s2 = fmaf(-m2, m2, acc[3][o]), s12 = fmaf(-m1, m2, acc[4][o]);
            const float rD2 = 1.f / (s1 + s2 + a.C2);
            const float cs = (2.f * s12 + a.C2) * rD2;
            float f = cs, ca = 2.f * (cs * m1 - m2) * rD2, cb = -2.f * cs * rD2, cc = 2.f * rD2;
            if (last) {
                const float rD1 = 1.f / (m1 * m1 + m2 * m2 + a.C1);
                const float l = (2.f * m1 * m2 + a.C1) * rD1;
                ca = cs * 2.f * (m2 - l * m1) * rD1 + l * ca;
                cb *= l;
                cc *= l;
                f = l * cs;
            }
            sum += f;
            if (A) {
                const int64_t j = (plane * H + qy) * W + qx;
                A[j] = ca;
                A[j + a.abc_stride] = cb;
                A[j + 2 * a.abc_stride] = cc;
            }
        }
    }
    const float r = block_sum<256>(sum, red);   // its barriers also fence this tile's reads of hp from the next pass
    if (threadIdx.x == 0) part[bid] = r;
  }
}

// One wave per plane: the tile partials of each scale in lane-strided order (the five scales' loads in flight
// together), vals[plane][s] = relu(scale mean), per_plane[plane] = prod vals^w.
__global__ __launch_bounds__(64) void msssim_fold_kernel(ms_fold_args a, const float* __restrict__ part,
                                                         float* __restrict__ vals, float* __restrict__ per_plane) {
    const int plane = blockIdx.x, lane = threadIdx.x;
    float acc[MS_SCALES];
#pragma unroll
    for (int s = 0; s < MS_SCALES; ++s) {
        const float* p = part + a.blk0[s] + (int64_t)plane * a.tiles[s];
        acc[s] = 0.f;
        for (int t = lane; t < a.tiles[s]; t += 64) acc[s] += p[t];
    }
    float ms = 1.f;
#pragma unroll
    for (int s = 0; s < MS_SCALES; ++s) {
        const float v = fmaxf(wave_sum(acc[s]) * a.inv_n[s], 0.f);
        ms *= powf(v, ms_weight(s));
        if (lane == 0) vals[plane * MS_SCALES + s] = v;
    }
    if (lane == 0) per_plane[plane] = ms;
}

// one block: the mean of the per-plane values in a fixed order
__global__ __launch_bounds__(256) void msssim_mean_kernel(const float* __restrict__ per_plane, int planes,
                                                          float* __restrict__ mean) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int p = threadIdx.x; p < planes; p += 256) acc += per_plane[p];
    const float r = block_sum<256>(acc, red);
    if (threadIdx.x == 0) *mean = r / (float)planes;
}

// tile t of one scale's backward grid (tiles over the input pixels): plane, origin and the plane's kappa
struct ms_bwd_tile {
    int p0y, p0x;
    int64_t plane;
    float kap;
    bool live;
};

__device__ __forceinline__ ms_bwd_tile ms_bwd_decode(const ms_bwd_args& a, int64_t t) {
    ms_bwd_tile c;
    const uint32_t plane = (uint32_t)t / (uint32_t)a.tiles, tile = (uint32_t)t - plane * (uint32_t)a.tiles;
    const uint32_t ty = tile / (uint32_t)a.tiles_x;   // the host keeps a scale's grid below 2^31 tiles
    c.plane = plane;
    c.p0y = (int)ty * MS_TILE;
    c.p0x = (int)(tile - ty * (uint32_t)a.tiles_x) * MS_TILE;
    // kappa_s = g / planes * w_s * ms_plane / v_s / n_s; exactly 0 for every scale of a plane the ReLU clamped
    float v[MS_SCALES];
    c.live = true;
#pragma unroll
    for (int i = 0; i < MS_SCALES; ++i) {
        v[i] = a.vals[c.plane * MS_SCALES + i];
        c.live = c.live && v[i] > 0.f;
    }
    c.kap = 0.f;
    if (c.live) {
        const float g = (a.g_mean ? *a.g_mean * a.inv_planes : 0.f) + (a.g_plane ? a.g_plane[c.plane] : 0.f);
        c.kap = g * a.coef * a.per_plane[c.plane] / ms_pick(v, a.scale);
    }
    return c;
}

// a, b, c at the 42 x 42 outputs q = p0 - 10 + (r, c) (zero outside the valid region), element threadIdx.x + 256 m
// in register m
__device__ __forceinline__ void ms_bwd_load(const ms_bwd_args& a, const ms_bwd_tile& c, float (&ra)[MS_LD],
                                            float (&rb)[MS_LD], float (&rc)[MS_LD]) {
    const int OH = a.H - MS_HALO, OW = a.W - MS_HALO;
    const float* __restrict__ A = a.abc + c.plane * a.H * a.W;
#pragma unroll
    for (int m = 0; m < MS_LD; ++m) {
        const int i = threadIdx.x + 256 * m;
        const int qy = c.p0y - MS_HALO + i / MS_IN, qx = c.p0x - MS_HALO + i % MS_IN;
        const bool ok = i < MS_IN * MS_IN && qy >= 0 && qy < OH && qx >= 0 && qx < OW;
        const int64_t j = (int64_t)qy * a.W + qx;
        ra[m] = ok ? A[j] : 0.f;
        rb[m] = ok ? A[j + a.abc_stride] : 0.f;
        rc[m] = ok ? A[j + 2 * a.abc_stride] : 0.f;
    }
}

// As the forward: a block walks tiles_per_block consecutive tiles and loads the next one while it filters this one.
__global__ __launch_bounds__(256) void msssim_bwd_kernel(ms_bwd_args a) {
    __shared__ float raw[3][MS_IN][MS_IN];
    __shared__ float hp[3][MS_IN][MS_TILE];
    const int H = a.H, W = a.W, ph = H & 1, pw = W & 1;
    const int col = threadIdx.x & 31, row0 = (threadIdx.x >> 5) * 4;
    const int64_t t_last = ((int64_t)blockIdx.x + 1) * a.tiles_per_block;
    const int64_t t_end = t_last < a.total_tiles ? t_last : a.total_tiles;
    ms_bwd_tile nxt = ms_bwd_decode(a, (int64_t)blockIdx.x * a.tiles_per_block);
    float ra[MS_LD], rb[MS_LD], rc[MS_LD];
    ms_bwd_load(a, nxt, ra, rb, rc);
    for (int64_t t = (int64_t)blockIdx.x * a.tiles_per_block; t < t_end; ++t) {
        const ms_bwd_tile cur = nxt;
        // this tile's X, Y and the coarser scale's gradient: in flight under the filter
        const int64_t pbase = cur.plane * H * W;
        float ex[4], ey[4], en[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int py = cur.p0y + row0 + o, px = cur.p0x + col;
            const bool ok = py < H && px < W;
            const int64_t j = pbase + (int64_t)py * W + px;
            ex[o] = ok ? a.x[j] : 0.f;
            ey[o] = ok ? a.y[j] : 0.f;
            en[o] = ok && a.dnext
                        ? a.dnext[cur.plane * a.Hn * a.Wn + (int64_t)((py + ph) >> 1) * a.Wn + ((px + pw) >> 1)]
                        : 0.f;
        }
#pragma unroll
        for (int m = 0; m < MS_LD; ++m) {
            const int i = threadIdx.x + 256 * m;
            if (i < MS_IN * MS_IN) {
                (&raw[0][0][0])[i] = ra[m];
                (&raw[1][0][0])[i] = rb[m];
                (&raw[2][0][0])[i] = rc[m];
            }
        }
        __syncthreads();
        if (t + 1 < t_end) {
            nxt = ms_bwd_decode(a, t + 1);
            ms_bwd_load(a, nxt, ra, rb, rc);
        }
        ms_hpass<3>(raw, hp);
        __syncthreads();   // also fences this pass's reads of raw from the next tile's stores
        float acc[3][4];
        ms_vpass<3>(hp, row0, col, acc);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int py = cur.p0y + row0 + o, px = cur.p0x + col;
            if (py < H && px < W) {
                float d = 0.25f * en[o];
                if (cur.live) d += cur.kap * (acc[0][o] + acc[1][o] * ex[o] + acc[2][o] * ey[o]);
                a.dx[pbase + (int64_t)py * W + px] = d;
            }
        }
        // the next tile's hp stores come after its barrier, which every thread reaches after these reads
    }
}

// ---------------------------------------------------------------------------
// host side: the scale geometry and the workspace layout (floats)
//   [X pyramid s = 1..4][Y pyramid][dX pyramid][vals planes x 5][partials, one per forward tile]
//   [a, b, c of every scale: 3 x planes x sum H_s W_s, only when the gradient is wanted]
// ---------------------------------------------------------------------------
struct ms_plan {
    int32_t H[MS_SCALES], W[MS_SCALES];
    int32_t tiles_x[MS_SCALES], tiles[MS_SCALES];
    int64_t blk0[MS_SCALES + 1];
    int64_t off[MS_SCALES + 1];        // planes * sum_{t < s} H_t W_t
    int64_t o_x, o_y, o_dx, o_vals, o_part, o_abc, total;
};

static bool ms_make_plan(int64_t planes, int32_t H, int32_t W, bool grad, ms_plan& p) {
    p.blk0[0] = 0;
    p.off[0] = 0;
    for (int s = 0; s < MS_SCALES; ++s) {
        p.H[s] = H;
        p.W[s] = W;
        if (H <= MS_HALO || W <= MS_HALO) return false;
        p.tiles_x[s] = (W - MS_HALO + MS_TILE - 1) / MS_TILE;
        const int64_t t = (int64_t)p.tiles_x[s] * ((H - MS_HALO + MS_TILE - 1) / MS_TILE);
        const int64_t in_t = (int64_t)((W + MS_TILE - 1) / MS_TILE) * ((H + MS_TILE - 1) / MS_TILE);
        if (in_t * planes > 0x7fffffff) return false;
        p.tiles[s] = (int32_t)t;
        p.blk0[s + 1] = p.blk0[s] + planes * t;
        p.off[s + 1] = p.off[s] + planes * H * W;
        H = H / 2 + H % 2;
        W = W / 2 + W % 2;
    }
    if (p.blk0[MS_SCALES] > 0x7fffffff) return false;
    const int64_t pyr = p.off[MS_SCALES] - p.off[1];
    p.o_x = 0;
    p.o_y = pyr;
    p.o_dx = 2 * pyr;
    p.o_vals = 3 * pyr;
    p.o_part = p.o_vals + planes * MS_SCALES;
    p.o_abc = p.o_part + p.blk0[MS_SCALES];
    p.total = p.o_abc + (grad ? 3 * p.off[MS_SCALES] : 0);
    return true;
}

static int ms_check(const char* what, int32_t planes, int32_t H, int32_t W, bool grad, const void* workspace,
                    size_t ws_bytes, ms_plan& p) {
    CAI_CHECK_ARG(planes > 0 && H > 0 && W > 0, "%s: planes %d, H %d, W %d must be positive", what, planes, H, W);
    CAI_CHECK_ARG(std::min(H, W) > MS_MIN_SIDE, "%s: image side must exceed %d for 5-scale MS-SSIM, got %d x %d", what,
                  MS_MIN_SIDE, H, W);
    CAI_CHECK_ARG(ms_make_plan(planes, H, W, grad, p), "%s: %d planes of %d x %d exceed the launch limits", what, planes,
                  H, W);
    CAI_CHECK_ARG(workspace && ws_bytes >= (size_t)p.total * sizeof(float), "%s: workspace of %zu bytes, need %zu", what,
                  workspace ? ws_bytes : (size_t)0, (size_t)p.total * sizeof(float));
    return CAI_OK;
}

static unsigned ms_ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

}  // namespace cai

using namespace cai;

extern "C" {

size_t cai_msssim_workspace_bytes(int32_t planes, int32_t H, int32_t W, int32_t with_grad) {
    ms_plan p;
    if (planes <= 0 || H <= 0 || W <= 0 || std::min(H, W) <= MS_MIN_SIDE || !ms_make_plan(planes, H, W, with_grad != 0, p)) {
        set_error("msssim_workspace_bytes: unsupported shape: %d planes of %d x %d (sides must exceed %d)", planes, H, W,
                  MS_MIN_SIDE);
        return 0;
    }
    return (size_t)p.total * sizeof(float);
}

int cai_msssim_fwd(const float* x, const float* y, int32_t planes, int32_t H, int32_t W, float data_range,
                   int32_t with_grad, float* per_plane, float* mean, void* workspace, size_t ws_bytes, void* stream) {
    CAI_CHECK_ARG(x && y && per_plane && mean, "msssim_fwd: null pointer");
    CAI_CHECK_ARG(data_range > 0.f, "msssim_fwd: data_range must be positive");
    ms_plan p;
    int rc = ms_check("msssim_fwd", planes, H, W, with_grad != 0, workspace, ws_bytes, p);
    if (rc) return rc;
    float* ws = reinterpret_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    ms_fwd_args a;
    ms_fold_args f;
    const int64_t all = p.off[MS_SCALES];
    for (int s = 0; s < MS_SCALES; ++s) {
        a.x[s] = s == 0 ? x : ws + p.o_x + (p.off[s] - p.off[1]);
        a.y[s] = s == 0 ? y : ws + p.o_y + (p.off[s] - p.off[1]);
        a.abc[s] = with_grad ? ws + p.o_abc + p.off[s] : nullptr;
        a.blk0[s] = f.blk0[s] = p.blk0[s];
        a.H[s] = p.H[s];
        a.W[s] = p.W[s];
        a.tiles_x[s] = p.tiles_x[s];
        a.tiles[s] = f.tiles[s] = p.tiles[s];
        f.inv_n[s] = (float)(1.0 / ((double)(p.H[s] - MS_HALO) * (p.W[s] - MS_HALO)));
    }
    a.abc_stride = all;
    a.C1 = (float)((0.01 * data_range) * (0.01 * data_range));
    a.C2 = (float)((0.03 * data_range) * (0.03 * data_range));
    for (int s = 0; s + 1 < MS_SCALES; ++s) {
        const int64_t n = (int64_t)planes * p.H[s + 1] * p.W[s + 1];
        hipLaunchKernelGGL(msssim_pool_kernel, dim3(ms_ew_grid(n)), dim3(256), 0, st, a.x[s], a.y[s],
                           const_cast<float*>(a.x[s + 1]), const_cast<float*>(a.y[s + 1]), (int64_t)planes, p.H[s], p.W[s],
                           p.H[s + 1], p.W[s + 1]);
    }
    float* part = ws + p.o_part;
    a.total_tiles = p.blk0[MS_SCALES];
    a.tiles_per_block = (int32_t)((a.total_tiles + MS_FWD_SLOTS - 1) / MS_FWD_SLOTS);
    const int64_t fwd_blocks = (a.total_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
    hipLaunchKernelGGL(msssim_fwd_kernel, dim3((unsigned)fwd_blocks), dim3(256), 0, st, a, part);
    hipLaunchKernelGGL(msssim_fold_kernel, dim3(planes), dim3(64), 0, st, f, part, ws + p.o_vals, per_plane);
    hipLaunchKernelGGL(msssim_mean_kernel, dim3(1), dim3(256), 0, st, per_plane, planes, mean);
    CAI_LAUNCH_CHECK("msssim_fwd");
    return CAI_OK;
}

int cai_msssim_bwd(const float* x, const float* y, int32_t planes, int32_t H, int32_t W, const float* per_plane,
                   const float* g_mean, const float* g_plane, float* dx, void* workspace, size_t ws_bytes,
                   void* stream) {
    CAI_CHECK_ARG(x && y && per_plane && dx, "msssim_bwd: null pointer");
    CAI_CHECK_ARG(g_mean || g_plane, "msssim_bwd: no upstream gradient");
    ms_plan p;
    int rc = ms_check("msssim_bwd", planes, H, W, true, workspace, ws_bytes, p);
    if (rc) return rc;
    float* ws = reinterpret_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    for (int s = MS_SCALES - 1; s >= 0; --s) {
        ms_bwd_args a;
        a.x = s == 0 ? x : ws + p.o_x + (p.off[s] - p.off[1]);
        a.y = s == 0 ? y : ws + p.o_y + (p.off[s] - p.off[1]);
        a.abc = ws + p.o_abc + p.off[s];
        a.abc_stride = p.off[MS_SCALES];
        a.vals = ws + p.o_vals;
        a.per_plane = per_plane;
        a.g_mean = g_mean;
        a.g_plane = g_plane;
        a.dnext = s == MS_SCALES - 1 ? nullptr : ws + p.o_dx + (p.off[s + 1] - p.off[1]);
        a.dx = s == 0 ? dx : ws + p.o_dx + (p.off[s] - p.off[1]);
        a.H = p.H[s];
        a.W = p.W[s];
        a.Hn = s == MS_SCALES - 1 ? 0 : p.H[s + 1];
        a.Wn = s == MS_SCALES - 1 ? 0 : p.W[s + 1];
        a.tiles_x = (p.W[s] + MS_TILE - 1) / MS_TILE;
        a.tiles = a.tiles_x * ((p.H[s] + MS_TILE - 1) / MS_TILE);
        a.scale = s;
        a.coef = (float)((double)ms_weight(s) / ((double)(p.H[s] - MS_HALO) * (p.W[s] - MS_HALO)));
        a.inv_planes = 1.f / (float)planes;
        a.total_tiles = (int64_t)a.tiles * planes;
        a.tiles_per_block = (int32_t)((a.total_tiles + MS_BWD_SLOTS - 1) / MS_BWD_SLOTS);
        const int64_t blocks = (a.total_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
        hipLaunchKernelGGL(msssim_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    }
    CAI_LAUNCH_CHECK("msssim_bwd");
    return CAI_OK;
}

}  // extern "C"
