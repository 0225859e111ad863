// mirt_trace_ray_text.inc -- the pieces of a ray query that every layout shares, as TEXT in parts (MIRT_TRACE_PART, in the manner of
// mirt_pool_hbm_schedule.inc): included by trace_rays_kernel and trace_rays_sorted_kernel (through mirt_trace_ray_body.inc) and by
// trace_rays_lds_kernel, with `i`, `alive` and `work` in scope.
//   MIRT_TRACE_SPHERES     the sphere table the flat scan reads: A.spheres in device memory, S.spheres staged
//   MIRT_TRACE_HIT_SPHERE  the hit's PreparedSphere
#if MIRT_TRACE_PART == 1       // the ray: two 16-byte loads
    trace_f4 r0 = { 0.0f, 0.0f, 0.0f, 0.0f }, r1 = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (alive) { r0 = rays[2u * i]; r1 = rays[2u * i + 1u]; }          // {origin, t_max} {direction, _pad}
    const f3 ro = mk(r0.x, r0.y, r0.z), rd = mk(r1.x, r1.y, r1.z);
    const float t_max = r0.w;
#elif MIRT_TRACE_PART == 2     // the flat scan: test_sphere in original index order from t_max, ANY leaves once no lane still looks
    const float a = dot(rd, rd);
    const float inv_a = rcp_(a);
    closest = t_max;
    best = -1;
    if (alive) work.add(kCntRays);
    const float4* sph = reinterpret_cast<const float4*>(MIRT_TRACE_SPHERES);      // {centre, r^2}: the first half of PreparedSphere i
    const uint32_t n = A.n_spheres;
    bool go = alive;
    for (uint32_t s = 0; s < n; ++s) {
        test_sphere<COUNT>(sph[2ull * s], s, ro, rd, a, inv_a, go, closest, best, work);
        if constexpr (ANY) {
            go = go && best < 0;
            if (!ballot_(go)) break;
        }
    }
#elif MIRT_TRACE_PART == 3     // the hit record: two 16-byte stores
    if (alive) {
        trace_u4 h0 = { 0u, kTraceMiss, 0u, 0u }, h1 = { 0u, 0u, 0u, 0u };
        if (best >= 0) {
            work.add(kCntHits);
            if constexpr (ANY) {
                h0.y = 0u;
            } else {
                // sphereIntersection (wgsl:431-440) as path_radiance computes it: the normal is not turned towards the ray
                const PreparedSphere sp = MIRT_TRACE_HIT_SPHERE;
                const f3 hp = fma3(closest, rd, ro);
                const f3 hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
                h0 = trace_u4{ bits(closest), (uint32_t)best, bits(hp.x), bits(hp.y) };
                h1 = trace_u4{ bits(hp.z), bits(hn.x), bits(hn.y), bits(hn.z) };
            }
        }
        hits[2u * i] = h0;
        hits[2u * i + 1u] = h1;
    }
#endif
