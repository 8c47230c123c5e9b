// rANS decoding, shared by the host coder (coder.cpp) and the fused autoregressive kernel (ar_coder.hip):
// 64-bit state, 32-bit words (third_party/ryg_rans/rans64.h:59-142), precision 16, and the escape scheme of
// cpp_exts/rans/rans_interface.cpp:231-281 (4-bit bypass nibbles, n_bypass <= 8).  Both sides include this
// file, so they decode the same symbols from the same bytes.  Plain inline functions, no allocation, no
// library calls; every loop is bounded by a constant or by the stream's length, every read by the stream's end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CAI_RANS_HD __host__ __device__ inline
#else
#define CAI_RANS_HD inline
#endif

namespace cai_rans {

constexpr uint32_t kScaleBits = 16;                 // rans_interface.cpp:49
constexpr uint32_t kBypassBits = 4;                 // rans_interface.cpp:51
constexpr uint32_t kMaxBypass = (1u << kBypassBits) - 1;
constexpr uint64_t kRansL = 1ull << 31;             // rans64.h:59

// outcome of a decode step (0 = fine); the host coder turns them into its messages, the kernel into the
// per-stream status word
enum Status : int32_t {
    kOk = 0,
    kTruncated = 1,     // truncated or corrupt stream
    kBadIndex = 2,      // cdf index out of range
    kBadCdfSize = 3,    // invalid cdf size for the index
    kBadLength = 4,     // stream length not a multiple of 4 / shorter than the 8-byte state / outside the buffer
};

struct DecState {
    uint64_t x = 0;
    const uint32_t* ptr = nullptr;
    const uint32_t* end = nullptr;
};

CAI_RANS_HD bool refill(DecState& d) {
    if (d.x < kRansL) {
        if (d.ptr >= d.end) return false;
        d.x = (d.x << 32) | *d.ptr++;
    }
    return true;
}

CAI_RANS_HD bool dec_init(DecState& d, const uint32_t* words, int64_t nwords) {
    if (nwords < 2) return false;
    d.x = (uint64_t)words[0] | ((uint64_t)words[1] << 32);
    d.ptr = words + 2;
    d.end = words + nwords;
    return true;
}

// rans_interface.cpp:89-105
CAI_RANS_HD bool get_bits(DecState& d, uint32_t nbits, uint32_t& val) {
    val = (uint32_t)(d.x & ((1u << nbits) - 1));
    d.x >>= nbits;
    return refill(d);
}

// First slot whose CDF value exceeds cum, minus one (the reference's linear find_if; a binary search on the
// non-decreasing table finds the same).
struct BinarySearch {
    CAI_RANS_HD int32_t operator()(const int32_t* cdf, int32_t size, uint32_t cum) const {
        int32_t lo = 0, n = size;
        while (n > 0) {   // <= 32 halvings
            const int32_t half = n >> 1;
            if (cdf[lo + half] <= (int32_t)cum) {
                lo += half + 1;
                n -= half + 1;
            } else {
                n = half;
            }
        }
        return lo - 1;
    }
};

// One symbol of rans_interface.cpp:231-281.  `find(cdf, size, cum)` returns the slot as BinarySearch does
// (the kernel searches with a whole wave).
template <typename Find>
CAI_RANS_HD int32_t decode_symbol(DecState& d, int32_t idx, const int32_t* cdfs, int64_t cdf_stride,
                                  const int32_t* cdf_sizes, const int32_t* offsets, int32_t n_cdfs, int32_t* out,
                                  Find find) {
    if (idx < 0 || idx >= n_cdfs) return kBadIndex;
    const int32_t* cdf = cdfs + (int64_t)idx * cdf_stride;
    const int32_t size = cdf_sizes[idx];
    const int32_t max_value = size - 2;
    if (max_value < 0 || max_value + 1 >= cdf_stride) return kBadCdfSize;
    const uint32_t cum = (uint32_t)(d.x & ((1u << kScaleBits) - 1));
    const int32_t s = find(cdf, size, cum);
    if (s < 0 || s >= size - 1) return kTruncated;
    const uint64_t start = (uint32_t)cdf[s], freq = (uint32_t)(cdf[s + 1] - cdf[s]);
    d.x = freq * (d.x >> kScaleBits) + (d.x & ((1u << kScaleBits) - 1)) - start;
    if (!refill(d)) return kTruncated;
    int32_t value = s;
    if (value == max_value) {
        uint32_t val;
        if (!get_bits(d, kBypassBits, val)) return kTruncated;
        int32_t n_bypass = (int32_t)val;
        // the count comes in 15-steps; a valid one never has a second step (n_bypass <= 8), a corrupt stream
        // ends this loop at its last word at the latest
        while (val == kMaxBypass) {
            if (!get_bits(d, kBypassBits, val)) return kTruncated;
            n_bypass += (int32_t)val;
        }
        if (n_bypass > 8) return kTruncated;
        uint32_t raw_val = 0;
        for (int32_t j = 0; j < n_bypass; ++j) {
            if (!get_bits(d, kBypassBits, val)) return kTruncated;
            raw_val |= val << (j * kBypassBits);
        }
        value = (int32_t)(raw_val >> 1);
        if (raw_val & 1)
            value = -value - 1;
        else
            value += max_value;
    }
    *out = value + offsets[idx];
    return kOk;
}

}  // namespace cai_rans
