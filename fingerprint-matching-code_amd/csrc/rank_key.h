// The ranking key: the one order behind everything the search side ranks (shortlists, prescreen, shard merge,
// subject fusion, open-set top-r, evaluation).
//
//   key = (order-preserving bits of the fp32 score) << 32 | (0xFFFFFFFF - index)
//
// Larger key = ranks earlier.  Scores descend; NaN ranks below every number (NaNs among themselves by index);
// -0 below +0; a tie goes to the lower index.  Keys of distinct indices are distinct, so "the k best" is "the k
// largest keys" with no tie logic and one answer whatever the schedule.  0 is below every key: an index is a
// non-negative int, so a key's index field is at least 2^31.  Every key is below 2^64 - 1: rank_bits never
// returns 0xFFFFFFFF (that would be the positive NaN pattern 0x7FFFFFFF, which maps to 0).
//
// The host statement is ops.rank_key; every kernel that ranks is tested bit for bit against it.
// Integer operations and shuffles only: the floating-point contraction mode of the including file does not matter.
#pragma once
#include "fpm_common.h"

namespace fpm {
typedef unsigned long long u64;

constexpr uint32_t QNAN_BITS = 0x7FC00000u;        // the canonical quiet NaN, the one NaN a kernel writes
__device__ __forceinline__ float qnan() { return __uint_as_float(QNAN_BITS); }

// fp32 bits -> unsigned, monotone in the value: negatives below positives (-0 below +0), NaN -> 0
// (below -inf, which maps to 0x007FFFFF)
__device__ __forceinline__ uint32_t rank_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 rank_key(float f, uint32_t index) {
    return ((u64)rank_bits(f) << 32) | (0xFFFFFFFFu - index);
}
__device__ __forceinline__ uint32_t rank_index(u64 key) { return 0xFFFFFFFFu - (uint32_t)key; }

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
// the largest v over a team of W adjacent lanes (W = 16 or 64), in every lane: the xor butterfly m = W/2, ..., 1
template <int W>
__device__ __forceinline__ u64 team_max_u64(u64 v) {
    static_assert(W == 16 || W == 64, "a team is 16 lanes or a whole wave");
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        const u64 o = shfl_xor_u64(v, m);
        v = o > v ? o : v;
    }
    return v;
}
}  // namespace fpm
