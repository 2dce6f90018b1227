// The order "nearest first" of Mash dist entries as one integer (mash_topk.hip, and the greedy
// selection of mash_dist.hip): by the exact rational common / denom, descending, 0 / 0 counting
// as 1; equal rationals by `pos`, ascending.
//   rank = 2^31 - floor(common * 2^31 / denom)   (0 for denom == 0),   key = rank << 32 | pos
// Two different fractions with denominators up to 2^14 differ by at least 2^-28, so their scaled
// values differ by at least 8 and the floors keep the order strictly; equal fractions give equal
// ranks.  The smaller key is the nearer entry.  No float arithmetic.
#pragma once
#include "common.hpp"

namespace hymet {

// the key of entry (common c, denom d) at position pos: c <= d <= 2^14
__device__ __forceinline__ uint64_t mash_rank_key(uint32_t c, uint32_t d, uint32_t pos) {
    uint32_t rank = 0;
    if (d != 0) {
        // floor(c * 2^31 / d) in two 32-bit divisions: c << 17 <= 2^31, the remainder is below 2^14
        const uint32_t hi = c << 17, q1 = hi / d, r1 = hi - q1 * d;
        rank = 0x80000000u - ((q1 << 14) + ((r1 << 14) / d));
    }
    return (uint64_t)rank << 32 | pos;
}

}  // namespace hymet
