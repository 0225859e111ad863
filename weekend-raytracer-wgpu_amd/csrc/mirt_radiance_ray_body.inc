// mirt_radiance_ray_body.inc -- the body of radiance_rays_kernel and radiance_rays_sorted_kernel (mirt_radiance_kernel.inc), included
// once by each with the macros of mirt_trace_ray_body.inc: MIRT_RAY_SLOT names the lane's slot in the launch (`i` itself in
// radiance_rays_kernel, which keeps the tokens and so the code object it had), MIRT_RAY_OF_SLOT is nothing or defines `i` from `slot`.
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
    trace_u4 r0 = { 0u, 0u, 0u, 0u }, r1 = { 0u, 0u, 0u, 0u };
    if (alive) { r0 = rays[2u * i]; r1 = rays[2u * i + 1u]; }          // {origin, stream} {direction, _pad}
    const f3 ro = mk(from_bits(r0.x), from_bits(r0.y), from_bits(r0.z));
    const f3 rd = mk(from_bits(r1.x), from_bits(r1.y), from_bits(r1.z));
    const uint32_t stream = r0.w;

    Work<false> work;
    work.clear();
    unsigned long long acc_r = 0, acc_g = 0, acc_b = 0;
    for (uint32_t s = 0; s < A.spp; ++s) {
        Rng rng;
        // generate_primary's seed with `stream` for the pixel index, then the two jitter and the two lens draws of a primary ray
        rng.state = jenkins_hash((stream ^ jenkins_hash(A.sample_begin + s + 1u)) ^ A.seed_mix);
        rng.skip(); rng.skip(); rng.skip(); rng.skip();
        const f3 c = path_radiance<false, HOSEK, false, SRC>(A, S, G, alive, rng, ro, rd, work, lane, nullptr, kNoCand, bvh_stack);
        acc_r += to_fixed(c.x);
        acc_g += to_fixed(c.y);
        acc_b += to_fixed(c.z);
    }
    if (alive) {
        uint32_t samples = A.spp;
        if (A.flags & kRadianceAccumulate) {
            const trace_u4 o0 = out[2u * i], o1 = out[2u * i + 1u];
            acc_r += (unsigned long long)o0.x | ((unsigned long long)o0.y << 32);
            acc_g += (unsigned long long)o0.z | ((unsigned long long)o0.w << 32);
            acc_b += (unsigned long long)o1.x | ((unsigned long long)o1.y << 32);
            samples += o1.z;
        }
        out[2u * i] = trace_u4{ (uint32_t)acc_r, (uint32_t)(acc_r >> 32), (uint32_t)acc_g, (uint32_t)(acc_g >> 32) };
        out[2u * i + 1u] = trace_u4{ (uint32_t)acc_b, (uint32_t)(acc_b >> 32), samples, 0u };
    }
