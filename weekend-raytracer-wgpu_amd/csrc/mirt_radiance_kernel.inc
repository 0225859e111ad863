// mirt_radiance_kernel.inc -- path-traced radiance for a caller's rays against a resident MIRT_SCENE_HBM scene
// (mirt_ctx_trace_radiance*; DESIGN.md 10.9).  Included once by mirt_kernels.hip behind mirt_feature_kernel.inc (it shares
// mirt_trace_kernel.inc's vector types), exact build only: there is no fast_build:: copy, no counting build and no dispenser.
//
// radiance_rays_kernel<HOSEK, BVH>: lane = ray, 64 consecutive rays per wave, ONE wave per block (kRadianceThreads), one ray per thread and no
// loop over rays: the caller's order is the wave's order (radiance_rays_sorted_kernel, MIRT_RADIANCE_SORT: the order of a permutation in
// device memory; the body of both is mirt_radiance_ray_body.inc).  RenderArgs.n_units is the number of rays; lanes of the last wave beyond it are
// not alive: they load nothing, take part in the wave's loops with their tests masked off and store nothing.  A ray (MirtRadianceRay,
// 32 bytes: {origin, stream} {direction, _pad}) is two 16-byte loads through a 4-byte-aligned vector type.
//   A sample is the renderer's sample from its primary ray on.  For s in sample_begin .. sample_begin + spp - 1 (the same trip count in
// every lane) the lane seeds the stream generate_primary would seed for a pixel whose index is the ray's `stream`, skips the four draws
// a primary ray consumes (two jitter, two lens) and calls path_radiance -- the function the render kernels call, with the source
// render_pt_hbm_kernel gives it -- from (origin, direction).  The three sums of to_fixed(radiance) are kept per lane as 64-bit
// integers; there is no reduction: a record depends on its ray alone.
//   BVH = true : kSrcBvh, nearest_hit_bvh through per_strip_args(), which is why RenderArgs is the FIRST kernel argument.  path_radiance
//                walks with the strip kernels' stack capacity, so every wave keeps kBvhStackBytesPerWave of traversal stacks in LDS.
//   BVH = false: kSrcHbmFlat, the flat scan of the sphere table in device memory (MIRT_RADIANCE_FLAT, the comparison build).
//   HOSEK      : the scene's sky blob, staged into LDS by stage_scene as in the render kernels.
// LDS of a block: stage_scene's image without the tables (the launch's camera words, which nothing reads, and the sky blob) | the wave's
// stacks, 8 KB.  Block size, measured (tools/radiance_rates.py, 1080p centre rays, 64- against 256-thread blocks, alternating runs;
// DESIGN.md 10.9): 484 spheres 2 / 16 spp 0.92 / 7.12 ms against 1.06 / 8.03, 1 M spheres 8.98 / 64.8 against 9.16 / 65.8, the same rays
// shuffled 18.8 / 147.6 against 28.0 / 222.1 -- a block leaves when its slowest wave is done and holds all its stacks until then, and
// with one wave per block LDS keeps 19 waves on a CU (160 KB / 8.1 KB) instead of 16 (four blocks of 32.1 KB), the residency of the
// render kernel's one-unit-per-wave launches.  The launch bounds ask for the 5 waves per SIMD that covers: 96 VGPRs allowed, 80 used.
//   A record (MirtRadiance, 32 bytes: three u64 sums, samples, _pad) leaves as two 16-byte stores; with MIRT_RADIANCE_ACCUMULATE
// (RenderArgs.flags, wave-uniform) two 16-byte loads precede them and the lane adds.

constexpr uint32_t kRadianceFlat = 1u << 0, kRadianceAccumulate = 1u << 1, kRadianceHosek = 1u << 2;     // MIRT_RADIANCE_* (include/mirt.h)
static_assert(kRadianceFlat == MIRT_RADIANCE_FLAT && kRadianceAccumulate == MIRT_RADIANCE_ACCUMULATE && kRadianceHosek == MIRT_RADIANCE_SKY_HOSEK,
              "RenderArgs.flags of a radiance launch are the caller's MIRT_RADIANCE_* bits");

template <bool HOSEK, bool BVH>
__global__ __launch_bounds__(kRadianceThreads, 5) void radiance_rays_kernel(RenderArgs A, const trace_u4* rays, trace_u4* out)
{
#define MIRT_RAY_SLOT i
#define MIRT_RAY_OF_SLOT
#include "mirt_radiance_ray_body.inc"
#undef MIRT_RAY_SLOT
#undef MIRT_RAY_OF_SLOT
}

// MIRT_RADIANCE_SORT (DESIGN.md 10.10): slot k of the launch loads and stores record order[k], the MIRT_RADIANCE_ACCUMULATE loads
// included -- the permutation ray_sort_order left in device memory.  The records stay where the caller put them.
template <bool HOSEK, bool BVH>
__global__ __launch_bounds__(kRadianceThreads, 5) void radiance_rays_sorted_kernel(RenderArgs A, const trace_u4* rays, trace_u4* out, const uint32_t* order)
{
#define MIRT_RAY_SLOT slot
#define MIRT_RAY_OF_SLOT const uint64_t i = alive ? order[slot] : 0u;
#include "mirt_radiance_ray_body.inc"
#undef MIRT_RAY_SLOT
#undef MIRT_RAY_OF_SLOT
}

static QueryKernel radiance_kernel(const QueryPlan& p)
{
    if (!p.sorted) return with_bools<QueryKernel>([](auto H, auto B) { return kernel_handle(radiance_rays_kernel<H.value, B.value>); }, p.hosek, p.bvh);
    return with_bools<QueryKernel>([](auto H, auto B) { return kernel_handle(radiance_rays_sorted_kernel<H.value, B.value>); }, p.hosek, p.bvh);
}
