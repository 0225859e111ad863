// mirt_trace_kernel.inc -- ray queries against a resident MIRT_SCENE_HBM scene (mirt_ctx_trace_rays*; DESIGN.md 10.7).  Included once by
// mirt_kernels.hip, exact build only: there is no fast_build:: copy.
//
// trace_rays_kernel<BVH, ANY, COUNT>: lane = ray, 64 consecutive rays per wave, kBlockThreads threads per block, one ray per thread and
// no loop over rays: the caller's order is the wave's order, nothing is sorted.  A ray (MirtRay, 32 bytes) is two 16-byte loads per
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
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const bool alive = i < n_rays;
    trace_f4 r0 = { 0.0f, 0.0f, 0.0f, 0.0f }, r1 = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (alive) { r0 = rays[2u * i]; r1 = rays[2u * i + 1u]; }          // {origin, t_max} {direction, _pad}
    const f3 ro = mk(r0.x, r0.y, r0.z), rd = mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w;

    Work<COUNT> work;
    work.clear();
    float closest;
    int best;
    if constexpr (BVH) {
        uint32_t* const stack = reinterpret_cast<uint32_t*>(smem) + (threadIdx.x >> 6) * (64u * A.bvh_stack_entries);
        best = nearest_hit_bvh<COUNT, ANY>(ro, rd, alive, closest, work, lane, stack, A.bvh_stack_entries, t_max);
    } else {
        const float a = dot(rd, rd);
        const float inv_a = rcp_(a);
        closest = t_max;
        best = -1;
        if (alive) work.add(kCntRays);
        const float4* sph = reinterpret_cast<const float4*>(A.spheres);      // {centre, r^2}: the first half of PreparedSphere i
        const uint32_t n = A.n_spheres;
        bool go = alive;
        for (uint32_t s = 0; s < n; ++s) {
            test_sphere<COUNT>(sph[2ull * s], s, ro, rd, a, inv_a, go, closest, best, work);
            if constexpr (ANY) {
                go = go && best < 0;
                if (!ballot_(go)) break;
            }
        }
    }
    if (alive) {
        trace_u4 h0 = { 0u, kTraceMiss, 0u, 0u }, h1 = { 0u, 0u, 0u, 0u };
        if (best >= 0) {
            work.add(kCntHits);
            if constexpr (ANY) {
                h0.y = 0u;
            } else {
                // sphereIntersection (wgsl:431-440) as path_radiance computes it: the normal is not turned towards the ray
                const PreparedSphere sp = A.spheres[best];
                const f3 hp = fma3(closest, rd, ro);
                const f3 hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
                h0 = trace_u4{ bits(closest), (uint32_t)best, bits(hp.x), bits(hp.y) };
                h1 = trace_u4{ bits(hp.z), bits(hn.x), bits(hn.y), bits(hn.z) };
            }
        }
        hits[2u * i] = h0;
        hits[2u * i + 1u] = h1;
    }
    work.flush(A.counters, lane);
}

using TraceKernel = void (*)(RenderArgs, const trace_f4*, trace_u4*, uint32_t);
static TraceKernel trace_kernel(bool bvh, bool any, bool count)
{
    if (bvh) return any ? (count ? trace_rays_kernel<true, true, true> : trace_rays_kernel<true, true, false>)
                        : (count ? trace_rays_kernel<true, false, true> : trace_rays_kernel<true, false, false>);
    return any ? (count ? trace_rays_kernel<false, true, true> : trace_rays_kernel<false, true, false>)
               : (count ? trace_rays_kernel<false, false, true> : trace_rays_kernel<false, false, false>);
}

// one thread per ray; a.lds_bytes = the block's traversal stacks (0 for the flat scan)
hipError_t launch_trace_rays(const RenderArgs& a, const void* d_rays, void* d_hits, uint32_t n_rays, bool bvh, bool any, bool count, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)n_rays + kBlockThreads - 1u) / kBlockThreads);
    hipLaunchKernelGGL(trace_kernel(bvh, any, count), dim3(blocks), dim3(kBlockThreads), a.lds_bytes, stream, a,
                       static_cast<const trace_f4*>(d_rays), static_cast<trace_u4*>(d_hits), n_rays);
    return hipGetLastError();
}
