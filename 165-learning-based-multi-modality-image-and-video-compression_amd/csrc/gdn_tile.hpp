// The lane-local GDN / IGDN forward step and its operand helpers, shared by the lane kernels (gdn_lane.hip)
// and by the conv kernels that run the GDN of their output (conv.hip, edge.hip).  gdn_lane.hip describes the
// operand layout; every user follows the same recipe, which makes its forward bit-identical to gdn_fwd_kernel:
// x rounded to bf16, x^2 = sq_chunk<bf16>(x), B operand = channels 32 kb + 8 (lane >> 4) .. +8 of pixel
// lane & 15, gamma A rows permuted by perm_ch, K blocks accumulated in order, then acc + beta, rsqrtf and
// x * rs (IGDN: x * nv * rs).
#pragma once

#include "common.hpp"
#include "mfma.hpp"

namespace cai {

// channel of row m of the gamma A fragment of output block cb
__device__ __forceinline__ int perm_ch(int cb, int m) { return 32 * (cb >> 1) + 8 * (m >> 2) + 4 * (cb & 1) + (m & 3); }

// The workgroup's copy of NM consecutive [C][C] bf16 matrices in LDS (rows padded by 16 bytes: the fragment reads
// of 16 rows at one column spread over the banks): one coalesced global read per workgroup instead of one
// fragment gather per wave.  Ends with a barrier.
template <int C, int NM, int NT>
__device__ __forceinline__ void stage_mats(char* lds, const bf16* mat) {
    constexpr int RSG = 2 * C + 16, CH = 2 * C / 16;   // row stride (bytes), 16-byte chunks per row
    for (int i = threadIdx.x; i < NM * C * CH; i += NT) {
        const int row = i / CH, ch = i - (i / CH) * CH;
        *reinterpret_cast<u32x4*>(lds + row * RSG + ch * 16) = *reinterpret_cast<const u32x4*>(mat + (int64_t)row * C + ch * 8);
    }
    __syncthreads();
}
template <int C>
__device__ __forceinline__ void afrag_lds(u32x4 (&a)[C / 16][C / 32], const char* img, int p, int g) {
    constexpr int RSG = 2 * C + 16;
#pragma unroll
    for (int cb = 0; cb < C / 16; ++cb) {
        const char* row = img + perm_ch(cb, p) * RSG + 16 * g;
#pragma unroll
        for (int kb = 0; kb < C / 32; ++kb) a[cb][kb] = *reinterpret_cast<const u32x4*>(row + 64 * kb);
    }
}

// One 16-pixel tile of the forward, output chunks kx0 .. kx0 + NKX - 1 (chunk kx = channels 32 kx + 8 g .. +8 of
// the lane's pixel): q = the squares of all C / 32 chunks (the B operand), xc the lane's bf16 chunks kx0 .. of x,
// ga the gamma fragments of output blocks 2 kx0 .. 2 (kx0 + NKX) - 1 (afrag_lds order), Lb beta in LDS; yv
// receives the output chunks in the layout of xc.  FENCE: a scheduling barrier after each chunk bounds the live
// accumulators (two waves per SIMD).
template <int C, bool INV, bool FENCE, int NKX>
__device__ __forceinline__ void gdn_tile_fwd_part(const u32x4 (&ga)[2 * NKX][C / 32], const float* Lb,
                                                  const u32x4 (&xc)[NKX], const u32x4 (&q)[C / 32], u32x4 (&yv)[NKX],
                                                  int g, int kx0) {
    constexpr int KB = C / 32;
#pragma unroll
    for (int kx = 0; kx < NKX; ++kx) {
        const bf16x8 xv = __builtin_bit_cast(bf16x8, xc[kx]);
        bf16x8 yy;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) acc = mma16<bf16>(ga[2 * kx + h][kb], q[kb], acc);
            const f32x4 bq = *reinterpret_cast<const f32x4*>(Lb + 32 * (kx0 + kx) + 8 * g + 4 * h);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float nv = acc[r] + bq[r];
                const float rs = rsqrtf(nv);
                yy[4 * h + r] = (bf16)((float)xv[4 * h + r] * (INV ? nv * rs : rs));
            }
        }
        yv[kx] = __builtin_bit_cast(u32x4, yy);
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
}
// all C / 32 chunks of the tile
template <int C, bool INV, bool FENCE>
__device__ __forceinline__ void gdn_tile_fwd(const u32x4 (&ga)[C / 16][C / 32], const float* Lb, const u32x4 (&xc)[C / 32],
                                             const u32x4 (&q)[C / 32], u32x4 (&yv)[C / 32], int g) {
    gdn_tile_fwd_part<C, INV, FENCE, C / 32>(ga, Lb, xc, q, yv, g, 0);
}

}  // namespace cai
