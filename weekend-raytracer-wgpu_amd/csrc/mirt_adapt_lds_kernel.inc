// mirt_adapt_lds_kernel.inc -- adaptive steps on a scene that lives in LDS (MIRT_ADAPT_LDS in MirtAdaptParams.flags; include/mirt.h,
// DESIGN.md 10.15).  Included once by mirt_kernels.hip behind mirt_adapt_pool_kernel.inc, exact build only.  The select stage is the one of
// mirt_adapt_kernel.inc; this file is the render stage:
//   adapt_pixels_lds_kernel<HOSEK, GRID>   256-thread blocks whose four waves share ONE staged scene -- stage_scene (+ stage_grid), what the
//                         strip kernel's lane-per-pixel builds stage, without the camera-ray candidate lists (listed pixels are no row runs).
//                         A PERSISTENT grid (the host does not know the count): min(ceil(pixels / 256), CUs x resident blocks) blocks, whose
//                         waves stride over the units, unit = blockIdx.x * 4 + wave, + gridDim.x * 4.  A block whose first unit does not
//                         exist returns before anything is staged; in a live block every wave passes the staging barriers and there is
//                         no block barrier behind them.
//                         A unit is 64 >> g consecutive list entries, their spp samples dealt to 1 << g groups of lanes (the strip
//                         kernel's px_groups, chosen ON THE DEVICE from the count: adapt_lds_groups of mirt_adapt_rule.h): lane l serves
//                         entry unit * (64 >> g) + (l & ((64 >> g) - 1)) as group l >> (6 - g), which takes samples n + grp * (spp >> g) ..
//                         of the pixel's stream.  The six 64-bit partial sums are added across the groups with wave shuffles and group
//                         0's lane adds them to the record and stores its four quads.  Integer sums: the split is invisible.
// The second build, adapt_pixels_lds_run_kernel<HOSEK, GRID>, reads a run's spp_j from count_word[1] (mirt_adapt_lds_text.inc).
//
// Registers (-Rpass-analysis=kernel-resource-usage, profiles/r20_adaptive_lds_resource_usage.txt): held to 4 waves per SIMD the eight builds
// take 79 (flat) / 89 (flat, Hosek) / 94 (grid) / 95 (grid, Hosek) VGPRs, no scratch and no spills: 6 / 5 / 5 / 5 waves per SIMD, i.e. as
// many 256-thread blocks per CU.  Held to 6 (-DMIRT_ADAPT_LDS_MINW=6, 80 VGPRs) the grid builds spill 15 registers and the flat Hosek
// build 5; only <false,false> fits as it is.  So the bound stays 4, and where LDS allows more blocks (mirt_adapt_lds_plan: up to 8) the
// occupancy answer is the smaller number.  A large flat table allows one or two blocks per CU: documented, not tuned.

#ifndef MIRT_ADAPT_LDS_MINW
#define MIRT_ADAPT_LDS_MINW 4                       // (experiment builds: -DMIRT_ADAPT_LDS_MINW=6)
#endif
constexpr uint32_t kAdaptLdsMinWaves = MIRT_ADAPT_LDS_MINW;     // waves per SIMD the builds are held to (launch bounds)

#define MIRT_ADAPT_LDS_KERNEL adapt_pixels_lds_kernel
#define MIRT_ADAPT_RUN 0
#include "mirt_adapt_lds_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_LDS_KERNEL
#define MIRT_ADAPT_LDS_KERNEL adapt_pixels_lds_run_kernel
#define MIRT_ADAPT_RUN 1
#include "mirt_adapt_lds_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_LDS_KERNEL

static QueryKernel adapt_lds_kernel(const QueryPlan& p)
{
    if (p.run) return with_bools<QueryKernel>([](auto H, auto G) { return kernel_handle(adapt_pixels_lds_run_kernel<H.value, G.value>); }, p.hosek, p.grid);
    return with_bools<QueryKernel>([](auto H, auto G) { return kernel_handle(adapt_pixels_lds_kernel<H.value, G.value>); }, p.hosek, p.grid);
}
