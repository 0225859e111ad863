// mirt_trace_ray_body.inc -- the body of trace_rays_kernel and trace_rays_sorted_kernel (mirt_trace_kernel.inc), included once by each
// with the two macros that say which record a lane works on:
//   MIRT_RAY_SLOT      the name of the lane's slot in the launch: `i` itself in trace_rays_kernel, whose tokens are then the ones the
//                      kernel had before the body moved here (its code object does not change); `slot` in the sorted kernel;
//   MIRT_RAY_OF_SLOT   nothing, or the statement that defines `i` from `slot` through the launch's permutation.
// A text include and not a __device__ function: the function, inlined, costs the existing kernels their register allocation (hipcc
// simplifies a callee on its own before it inlines it; DESIGN.md 10.10 has the figures).
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t MIRT_RAY_SLOT = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const bool alive = MIRT_RAY_SLOT < n_rays;
    MIRT_RAY_OF_SLOT
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
