// mirt_trace_ray_body.inc -- what is trace_rays_kernel's and trace_rays_sorted_kernel's own (mirt_trace_kernel.inc): the lane's record, the
// BVH walk and the counters' flush; the ray load, the flat scan and the hit record are mirt_trace_ray_text.inc's parts.  Included once by
// each kernel with the two macros that say which record a lane works on:
//   MIRT_RAY_SLOT      the name of the lane's slot in the launch: `i` itself in trace_rays_kernel, whose tokens are then the ones the
//                      kernel had before the body moved here (its code object does not change); `slot` in the sorted kernel;
//   MIRT_RAY_OF_SLOT   nothing, or the statement that defines `i` from `slot` through the launch's permutation.
// A text include and not a __device__ function: the function, inlined, costs the existing kernels their register allocation (hipcc
// simplifies a callee on its own before it inlines it; DESIGN.md 10.10 has the figures).
#define MIRT_TRACE_SPHERES A.spheres
#define MIRT_TRACE_HIT_SPHERE A.spheres[best]
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t MIRT_RAY_SLOT = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const bool alive = MIRT_RAY_SLOT < n_rays;
    MIRT_RAY_OF_SLOT
#define MIRT_TRACE_PART 1
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART

    Work<COUNT> work;
    work.clear();
    float closest;
    int best;
    if constexpr (BVH) {
        uint32_t* const stack = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (64u * A.bvh_stack_entries);
        best = nearest_hit_bvh<COUNT, ANY>(ro, rd, alive, closest, work, lane, stack, A.bvh_stack_entries, t_max);
    } else {
#define MIRT_TRACE_PART 2
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART
    }
#define MIRT_TRACE_PART 3
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART
    work.flush(A.counters, lane);
#undef MIRT_TRACE_SPHERES
#undef MIRT_TRACE_HIT_SPHERE
