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

// The step size of an adaptive RUN (mirt_ctx_adapt_run_device), ONE function for the host (mirt_adapt_run_spp) and the
// device (thread 0 of adapt_scan_run_kernel): a step that lists `count` pixels takes base << k samples of each, k the smallest for which
// count x (base << k) reaches min_items or base << k is the cap (cap = base << m, or 0 for base: the caller has checked it).  The
// product is 64 bit: count < 2^32 and base << k <= cap <= 2^24.
__host__ __device__ inline uint32_t adapt_run_spp(uint32_t count, uint32_t base, uint32_t min_items, uint32_t cap)
{
    if (count == 0u) return 0u;
    if (cap == 0u) cap = base;
    uint32_t spp = base;
    while ((uint64_t)count * spp < (uint64_t)min_items && spp < cap) spp <<= 1;
    return spp;
}

// The sample groups of an MIRT_ADAPT_LDS step (adapt_pixels_lds_kernel), ONE function for the host (mirt_adapt_lds_groups)
// and the device (every wave of the render stage): a unit is 64 >> g list entries, whose spp samples are dealt to 1 << g groups of lanes.
// g is the smallest of 0 .. g_cap = min(2, trailing zero bits of spp) that gives each of the grid's `grid_waves` waves a unit, or g_cap
// where none does; an empty list takes g = 0.  spp == 0 (an empty step of a run) has g_cap 0.
__host__ __device__ inline uint32_t adapt_lds_groups(uint32_t count, uint32_t spp, uint32_t grid_waves)
{
    if (count == 0u) return 0u;
    const uint32_t g_cap = (spp & 1u) || spp == 0u ? 0u : (spp & 2u) ? 1u : 2u;
    for (uint32_t g = 0; g < g_cap; ++g) {
        const uint32_t px = 64u >> g;
        if (count / px + (count % px != 0u ? 1u : 0u) >= grid_waves) return g;
    }
    return g_cap;
}

}  // namespace mirt
