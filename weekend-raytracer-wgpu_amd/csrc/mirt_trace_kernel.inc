// mirt_trace_kernel.inc -- ray queries against a resident MIRT_SCENE_HBM scene (mirt_ctx_trace_rays*; DESIGN.md 10.7).  Included once by
// mirt_kernels.hip, exact build only: there is no fast_build:: copy.
//
// trace_rays_kernel<BVH, ANY, COUNT>: lane = ray, 64 consecutive rays per wave, kBlockThreads threads per block, one ray per thread and
// no loop over rays: the caller's order is the wave's order (trace_rays_sorted_kernel, MIRT_RAYS_SORT: the order of a permutation in
// device memory; the body of both is mirt_trace_ray_body.inc).  A ray (MirtRay, 32 bytes) is two 16-byte loads per
// lane, a hit (MirtRayHit, 32 bytes) two 16-byte stores; consecutive lanes touch consecutive 32-byte records.  The caller's pointers
// are only 4-byte aligned by contract, hence the vector type below.  Lanes of the last wave beyond n_rays are not alive: they load
// nothing, take part in the wave's loops with their tests masked off, and store nothing.
//   BVH   = true : nearest_hit_bvh itself -- the function of the render kernels, started at the ray's t_max instead of kMaxT.  It reads
//                  the tree through per_strip_args(), i.e. from the start of the kernarg segment, which is why RenderArgs is the FIRST
//                  kernel argument (filled by the host code of the render launch, mirt_api.hip: fill_bvh_args).  Traversal stacks: 64 per
//                  wave of RenderArgs.bvh_stack_entries node references -- the resident tree's depth --, lane-interleaved, dynamic LDS.
//   BVH   = false: the flat scan, test_sphere over the prepared sphere table in ORIGINAL index order (the tie-break's order), the
//                  comparison build (MIRT_RAYS_FLAT).  The records' addresses are wave-uniform.
//   ANY   = true : a lane stops at the first sphere with f < t_max; the record says hit (sphere = 0) or miss, everything else 0.
//   COUNT = true : Work<true>: rays, sphere tests a lane really performs, roots, rays with a hit, BVH nodes visited per lane / per wave.
typedef float    trace_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t trace_u4 __attribute__((ext_vector_type(4), aligned(4)));      // a hit record travels as bit patterns (MIRT_RAY_MISS is a NaN's)

constexpr uint32_t kTraceMiss = MIRT_RAY_MISS;

template <bool BVH, bool ANY, bool COUNT>
__global__ __launch_bounds__(kBlockThreads) void trace_rays_kernel(RenderArgs A, const trace_f4* rays, trace_u4* hits, uint32_t n_rays)
{
#define MIRT_RAY_SLOT i
#define MIRT_RAY_OF_SLOT
#include "mirt_trace_ray_body.inc"
#undef MIRT_RAY_SLOT
#undef MIRT_RAY_OF_SLOT
}

// MIRT_RAYS_SORT (DESIGN.md 10.10): the same lanes and waves, but slot k of the launch loads and stores record order[k] -- the
// permutation ray_sort_order left in device memory, ascending (code, caller's index).  The records stay where the caller put them.
template <bool BVH, bool ANY, bool COUNT>
__global__ __launch_bounds__(kBlockThreads) void trace_rays_sorted_kernel(RenderArgs A, const trace_f4* rays, trace_u4* hits, uint32_t n_rays, const uint32_t* order)
{
#define MIRT_RAY_SLOT slot
#define MIRT_RAY_OF_SLOT const uint64_t i = alive ? order[slot] : 0u;
#include "mirt_trace_ray_body.inc"
#undef MIRT_RAY_SLOT
#undef MIRT_RAY_OF_SLOT
}

static QueryKernel trace_kernel(const QueryPlan& p)
{
    if (!p.sorted) return with_bools<QueryKernel>([](auto B, auto A, auto C) { return kernel_handle(trace_rays_kernel<B.value, A.value, C.value>); }, p.bvh, p.any, p.count);
    return with_bools<QueryKernel>([](auto B, auto A, auto C) { return kernel_handle(trace_rays_sorted_kernel<B.value, A.value, C.value>); }, p.bvh, p.any, p.count);
}

