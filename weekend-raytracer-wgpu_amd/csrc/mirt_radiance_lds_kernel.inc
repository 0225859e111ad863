// mirt_radiance_lds_kernel.inc -- path-traced radiance for a caller's rays against a scene that lives in LDS (MIRT_QUERY_LDS in
// MirtRadianceParams.flags; include/mirt.h, DESIGN.md 10.16).  Included once by mirt_kernels.hip behind the MIRT_SCENE_HBM query kernels,
// whose vector types and flag constants it shares; exact build only.
//
// radiance_rays_lds_kernel<HOSEK, GRID>: the shape of adapt_pixels_lds_kernel (mirt_adapt_lds_kernel.inc) -- 256-thread blocks whose four
// waves share ONE staged scene, a persistent grid of min(ceil(rays / 256), CUs x resident blocks) blocks whose waves stride over units
// of 64 consecutive rays, unit = blockIdx.x * 4 + wave, + gridDim.x * 4: lane = ray, the wave composition of radiance_rays_kernel.
// RenderArgs.n_units is the number of rays.  A block whose first unit does not exist returns before anything is staged; in a live block
// every wave passes the staging barriers and there is no block barrier behind them.
// The ray body is mirt_radiance_ray_body.inc's: the stream seeded from the ray's `stream` word, the four draws of a primary ray skipped,
// path_radiance from (origin, direction) -- here <false, HOSEK, GRID, kSrcLds> without a candidate list, as the LDS adaptive step calls
// it --, three 64-bit integer sums per lane, and with MIRT_RADIANCE_ACCUMULATE the record's loads before its stores.

template <bool HOSEK, bool GRID>
__global__ __launch_bounds__(kQueryLdsThreads, kQueryLdsMinWaves) void radiance_rays_lds_kernel(RenderArgs A, const trace_u4* rays, trace_u4* out)
{
    constexpr uint32_t kWaves = kQueryLdsThreads / 64u;
    const uint32_t n_rays = A.n_units;
    const uint32_t units = n_rays / 64u + (n_rays % 64u != 0u ? 1u : 0u);
    if (blockIdx.x * kWaves >= units) return;                               // the whole block: nothing staged, no barrier met
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, !GRID>(A, smem, HOSEK);
    GridLds G{};
    if constexpr (GRID) G = stage_grid(A, smem + scene_lds_bytes_dev(A.n_spheres, A.n_mats, HOSEK, false));
    // no block barrier from here on: a wave without units leaves, the others stride over theirs
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t grid_waves = gridDim.x * kWaves;
    Work<false> work;
    work.clear();
    for (uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); unit < units; unit += grid_waves) {
        const uint64_t i = (uint64_t)unit * 64u + lane;
        const bool alive = i < n_rays;
        trace_u4 r0 = { 0u, 0u, 0u, 0u }, r1 = { 0u, 0u, 0u, 0u };
        if (alive) { r0 = rays[2u * i]; r1 = rays[2u * i + 1u]; }          // {origin, stream} {direction, _pad}
        const f3 ro = mk(from_bits(r0.x), from_bits(r0.y), from_bits(r0.z));
        const f3 rd = mk(from_bits(r1.x), from_bits(r1.y), from_bits(r1.z));
        const uint32_t stream = r0.w;

        unsigned long long acc_r = 0, acc_g = 0, acc_b = 0;
        for (uint32_t s = 0; s < A.spp; ++s) {
            Rng rng;
            // generate_primary's seed with `stream` for the pixel index, then the two jitter and the two lens draws of a primary ray
            rng.state = jenkins_hash((stream ^ jenkins_hash(A.sample_begin + s + 1u)) ^ A.seed_mix);
            rng.skip(); rng.skip(); rng.skip(); rng.skip();
            const f3 c = path_radiance<false, HOSEK, GRID, kSrcLds>(A, S, G, alive, rng, ro, rd, work, lane, nullptr, kNoCand, nullptr);
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
    }
}

static QueryKernel radiance_lds_kernel(const QueryPlan& p)
{
    return with_bools<QueryKernel>([](auto H, auto G) { return kernel_handle(radiance_rays_lds_kernel<H.value, G.value>); }, p.hosek, p.grid);
}
