// mirt_radiance_lds_kernel.inc -- path-traced radiance for a caller's rays against a scene that lives in LDS (MIRT_QUERY_LDS in
// MirtRadianceParams.flags; include/mirt.h, DESIGN.md 10.16).  Included once by mirt_kernels.hip behind the MIRT_SCENE_HBM query kernels,
// whose vector types and flag constants it shares; exact build only.
//
// radiance_rays_lds_kernel<HOSEK, GRID>: the shape of adapt_pixels_lds_kernel (mirt_adapt_lds_kernel.inc) -- 256-thread blocks whose four
// waves share ONE staged scene, a persistent grid of min(ceil(rays / 256), CUs x resident blocks) blocks whose waves stride over units
// of 64 consecutive rays, unit = blockIdx.x * 4 + wave, + gridDim.x * 4: lane = ray, the wave composition of radiance_rays_kernel.
// RenderArgs.n_units is the number of rays.  A block whose first unit does not exist returns before anything is staged; in a live block
// every wave passes the staging barriers and there is no block barrier behind them.
// The block begins with mirt_lds_block_text.inc; a ray is mirt_radiance_item_text.inc, the text radiance_rays_kernel includes, with
// path_radiance<false, HOSEK, GRID, kSrcLds> without a candidate list and without a stack, as the LDS adaptive step calls it.

template <bool HOSEK, bool GRID>
__global__ __launch_bounds__(kQueryLdsThreads, kQueryLdsMinWaves) void radiance_rays_lds_kernel(RenderArgs A, const trace_u4* rays, trace_u4* out)
{
    constexpr uint32_t kWaves = kQueryLdsThreads / 64u;
    const uint32_t n_rays = A.n_units;
    const uint32_t units = n_rays / 64u + (n_rays % 64u != 0u ? 1u : 0u);
#define MIRT_LDS_SKY HOSEK
#include "mirt_lds_block_text.inc"
#undef MIRT_LDS_SKY
    const uint32_t grid_waves = gridDim.x * kWaves;
    Work<false> work;
    work.clear();
    for (uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); unit < units; unit += grid_waves) {
        const uint64_t i = (uint64_t)unit * 64u + lane;
        const bool alive = i < n_rays;
#define MIRT_RADIANCE_GRID GRID
#define MIRT_RADIANCE_SRC kSrcLds
#define MIRT_RADIANCE_STACK nullptr
#include "mirt_radiance_item_text.inc"
#undef MIRT_RADIANCE_GRID
#undef MIRT_RADIANCE_SRC
#undef MIRT_RADIANCE_STACK
    }
}

static QueryKernel radiance_lds_kernel(const QueryPlan& p)
{
    return with_bools<QueryKernel>([](auto H, auto G) { return kernel_handle(radiance_rays_lds_kernel<H.value, G.value>); }, p.hosek, p.grid);
}
