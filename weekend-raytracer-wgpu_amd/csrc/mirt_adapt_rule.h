// mirt_adapt_rule.h -- the stopping rule of adaptive sampling (include/mirt.h, mirt_ctx_adapt_*), ONE function for the
// host (mirt_adapt_active, mirt_api.hip) and the device (adapt_select_kernel, mirt_adapt_kernel.inc), so that the two agree on every
// record by construction.  Exact for every bit pattern of a record: |2 even - sum| < 2^65, e < 3 x 2^65, e x 2^16 < 2^83; m < 3 x 2^64,
// n x 2^17 < 2^49, times a 32-bit tolerance < 2^98 -- all of it fits 128 bits.
#pragma once

#include <stdint.h>

#include "../../include/mirt.h"

namespace mirt {

__host__ __device__ inline bool adapt_active(const uint64_t sum[3], const uint64_t even[3], uint32_t n, const MirtAdaptParams& P)
{
    typedef unsigned __int128 u128;
    if (n >= P.max_samples) return false;
    if (n < P.min_samples || n < 2u) return true;
    u128 e = 0, m = 0;
    for (int k = 0; k < 3; ++k) {
        const u128 twice = (u128)even[k] << 1, s = (u128)sum[k];
        e += twice > s ? twice - s : s - twice;
        m += s;
    }
    const bool converged = (e << 16) <= (u128)P.tolerance * (m + (u128)n * MIRT_ADAPT_FLOOR);
    return !converged;
}

}  // namespace mirt
