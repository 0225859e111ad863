// mirt_radiance_ray_body.inc -- what is radiance_rays_kernel's and radiance_rays_sorted_kernel's own (mirt_radiance_kernel.inc): the
// staging, the wave's stacks and the lane's record; the ray itself is mirt_radiance_item_text.inc.  Included once by each kernel with the
// macros of mirt_trace_ray_body.inc: MIRT_RAY_SLOT names the lane's slot in the launch (`i` itself in radiance_rays_kernel, which keeps
// the tokens and so the code object it had), MIRT_RAY_OF_SLOT is nothing or defines `i` from `slot`.
    constexpr uint32_t SRC = BVH ? kSrcBvh : kSrcHbmFlat;
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, false>(A, smem, HOSEK);
    const GridLds G{};
    uint32_t* bvh_stack = nullptr;
    if constexpr (BVH)
        bvh_stack = reinterpret_cast<uint32_t*>(smem + scene_lds_bytes_dev(A.n_spheres, A.n_mats, HOSEK, false)) + (threadIdx.x >> 6) * (kBvhStackBytesPerWave / 4u);      // (one wave per block today: + 0)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t MIRT_RAY_SLOT = (uint64_t)blockIdx.x * kRadianceThreads + threadIdx.x;
    const bool alive = MIRT_RAY_SLOT < A.n_units;
    MIRT_RAY_OF_SLOT
    Work<false> work;
    work.clear();
#define MIRT_RADIANCE_GRID false
#define MIRT_RADIANCE_SRC SRC
#define MIRT_RADIANCE_STACK bvh_stack
#include "mirt_radiance_item_text.inc"
#undef MIRT_RADIANCE_GRID
#undef MIRT_RADIANCE_SRC
#undef MIRT_RADIANCE_STACK
