// mirt_adapt_pixels_text.inc -- the render stage of an unpooled adaptive step, as TEXT: mirt_adapt_kernel.inc includes it twice.
//   MIRT_ADAPT_PIXELS_KERNEL   the kernel's name: adapt_pixels_kernel (a step) or adapt_pixels_run_kernel (a step of a run)
//   MIRT_ADAPT_RUN             0: the lane's sample count is the launch's, A.spp
//                              1: it is the word behind the count (head[1], which adapt_scan_run_kernel wrote for this step), read as a
//                                 wave-uniform word next to the count, before anything is staged (DESIGN.md 10.14)
// Text and not a template parameter: adapt_pixels_kernel<HOSEK, BVH> keeps its name and, token for token, its code.
template <bool HOSEK, bool BVH>
__global__ __launch_bounds__(kAdaptThreads, 5) void MIRT_ADAPT_PIXELS_KERNEL(RenderArgs A, adapt_u4* recs, const uint32_t* list, const uint32_t* count_word)
{
    constexpr uint32_t SRC = BVH ? kSrcBvh : kSrcHbmFlat;
    const uint32_t count = __builtin_amdgcn_readfirstlane(*count_word);
#if MIRT_ADAPT_RUN
    const uint32_t step_spp = __builtin_amdgcn_readfirstlane(count_word[1]);      // 0 exactly when count is 0
#define MIRT_ADAPT_SPP(ARGS) ((void)(ARGS), step_spp)
#else
#define MIRT_ADAPT_SPP(ARGS) (ARGS).spp
#endif
    if (blockIdx.x * kAdaptThreads >= count) return;                   // the whole block (one wave): nothing staged, no barrier met
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, false>(A, smem, HOSEK);
    const GridLds G{};
    uint32_t* bvh_stack = nullptr;
    if constexpr (BVH)
        bvh_stack = reinterpret_cast<uint32_t*>(smem + scene_lds_bytes_dev(A.n_spheres, A.n_mats, HOSEK, false)) + (threadIdx.x >> 6) * (kBvhStackBytesPerWave / 4u);      // (one wave per block: + 0)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = blockIdx.x * kAdaptThreads + threadIdx.x;    // < 2^32: the grid covers out_rows x width <= 2^32 - 1 pixels
    const bool alive = slot < count;
    const uint64_t pi = alive ? list[slot] : 0u;                       // the record's place in the band; < out_rows x width (adapt_compact_kernel)
    const uint32_t ci = (uint32_t)pi / A.width;
    const uint32_t x = (uint32_t)pi - ci * A.width;
    const uint32_t y = abs_row(A, ci);
    adapt_u4 q0 = { 0u, 0u, 0u, 0u }, q1 = q0, q2 = q0, q3 = q0;
    if (alive) { q0 = recs[4u * pi]; q1 = recs[4u * pi + 1u]; q2 = recs[4u * pi + 2u]; q3 = recs[4u * pi + 3u]; }
    const uint32_t n = q3.x;

    Work<false> work;
    work.clear();
    unsigned long long sum_r = adapt_u64(q0.x, q0.y), sum_g = adapt_u64(q0.z, q0.w), sum_b = adapt_u64(q1.x, q1.y);
    unsigned long long even_r = adapt_u64(q1.z, q1.w), even_g = adapt_u64(q2.x, q2.y), even_b = adapt_u64(q2.z, q2.w);
    for (uint32_t s = 0; s < MIRT_ADAPT_SPP(A); ++s) {
        Rng rng;
        f3 ro, rd;
        {   // camera constants are re-read from LDS per sample instead of living in 21 VGPRs (strip_kernel_body)
            const CamRegs C = load_camera(S, A);
            generate_primary(A, C, x, y, n + s, rng, ro, rd);
        }
        const f3 c = path_radiance<false, HOSEK, false, SRC>(A, S, G, alive, rng, ro, rd, work, lane, nullptr, kNoCand, bvh_stack);
        const unsigned long long fr = to_fixed(c.x), fg = to_fixed(c.y), fb = to_fixed(c.z);
        sum_r += fr; sum_g += fg; sum_b += fb;
        if (((n + s) & 1u) == 0u) { even_r += fr; even_g += fg; even_b += fb; }
    }
    if (alive) {
        recs[4u * pi] = adapt_u4{ (uint32_t)sum_r, (uint32_t)(sum_r >> 32), (uint32_t)sum_g, (uint32_t)(sum_g >> 32) };
        recs[4u * pi + 1u] = adapt_u4{ (uint32_t)sum_b, (uint32_t)(sum_b >> 32), (uint32_t)even_r, (uint32_t)(even_r >> 32) };
        recs[4u * pi + 2u] = adapt_u4{ (uint32_t)even_g, (uint32_t)(even_g >> 32), (uint32_t)even_b, (uint32_t)(even_b >> 32) };
        recs[4u * pi + 3u] = adapt_u4{ n + MIRT_ADAPT_SPP(A), 0u, 0u, 0u };
    }
}
#undef MIRT_ADAPT_SPP
