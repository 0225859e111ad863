// mirt_feature_lds_kernel.inc -- first-hit feature frames of a scene that lives in LDS (MIRT_QUERY_LDS in the flags of
// mirt_ctx_render_features*; include/mirt.h, DESIGN.md 10.16).  Included once by mirt_kernels.hip behind the MIRT_SCENE_HBM query kernels,
// whose vector types and helpers (feature_camera, kTraceMiss) it shares; exact build only.
//
// feature_frame_lds_kernel<GRID>: the shape of adapt_pixels_lds_kernel (mirt_adapt_lds_kernel.inc) -- 256-thread blocks whose four waves
// share ONE staged scene, a persistent grid of min(ceil(pixels / 256), CUs x resident blocks) blocks whose waves stride over units of 64
// consecutive COMPACT pixels, unit = blockIdx.x * 4 + wave, + gridDim.x * 4: lane = pixel, the wave composition of feature_frame_kernel.
// A block whose first unit does not exist returns before anything is staged; in a live block every wave passes the staging barriers and
// there is no block barrier behind them.
// The block begins with mirt_lds_block_text.inc; a pixel is mirt_feature_item_text.inc, the text feature_frame_kernel includes -- centre
// ray first, then the sample set, float sums from +0 -- with this layout's nearest hit:
//   GRID = false: nearest_hit over the staged sphere table, original index order (the strip kernels' flat scan);
//   GRID = true : nearest_hit_grid, the strip kernels' walk, two-dimensional where the grid is one cell high.
// Both start at kMaxT and are held to the flat scan of the HBM build bit for bit (test_sphere's (f, id) tie-break and the builder's
// slack; tests/test_gpu_grid_rounding.py).  A hit's PreparedSphere comes from the staged table (flat) or from device memory (grid: one
// read per hit, as path_radiance does), its material from S.pmats.
//
// Registers (-Rpass-analysis=kernel-resource-usage, profiles/r24_query_lds_resource_usage.txt): the builds are held to 4 waves per SIMD,
// as the adaptive LDS step is (kQueryLdsMinWaves, mirt_trace_lds_kernel.inc); none uses scratch.

template <bool GRID>
MIRT_DEV int feature_nearest_hit_lds(const RenderArgs& A, const SceneLds& S, const GridLds& G, f3 ro, f3 rd, bool alive, float& closest, Work<false>& work, uint32_t lane)
{
    if constexpr (GRID) {
        return A.grid_flat_y ? nearest_hit_grid<false, true>(S, G, ro, rd, alive, closest, work, lane)
                             : nearest_hit_grid<false, false>(S, G, ro, rd, alive, closest, work, lane);
    } else {
        return nearest_hit<false>(S, A.n_spheres, ro, rd, alive, closest, work);
    }
}

// feature_of_hit (mirt_feature_kernel.inc) with the tables where this layout keeps them; a fix to one is a fix to both
template <bool GRID>
MIRT_DEV void feature_of_hit_lds(const RenderArgs& A, const SceneLds& S, int best, float t, f3 ro, f3 rd, f3& hn, f3& albedo)
{
    PreparedSphere sp;
    if constexpr (GRID) sp = A.spheres[best];
    else sp = S.spheres[best];
    const f3 hp = fma3(t, rd, ro);
    hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
    const PreparedMaterial* m = &S.pmats[sp.material_idx];
    switch (m->id) {
    case 0u:
    case 1u: albedo = albedo_at(A, m, 0, hn); break;
    case 2u: albedo = mk(1, 1, 1); break;
    case 3u: albedo = albedo_at(A, m, sin_product_negative(5.0f * hp.x, 5.0f * hp.y, 5.0f * hp.z) ? 0 : 1, hn); break;
    default: albedo = mk(0.9921f, 0.24705f, 0.57254f); break;
    }
}

template <bool GRID>
__global__ __launch_bounds__(kQueryLdsThreads, kQueryLdsMinWaves) void feature_frame_lds_kernel(RenderArgs A, trace_u4* out)
{
    constexpr uint32_t kWaves = kQueryLdsThreads / 64u;
    const uint64_t n_pix = (uint64_t)A.out_rows * A.width;                  // < 2^32 (check_features)
    const uint32_t units = (uint32_t)((n_pix + 63u) / 64u);
#define MIRT_LDS_SKY false
#include "mirt_lds_block_text.inc"
#undef MIRT_LDS_SKY
    const uint32_t grid_waves = gridDim.x * kWaves;
    const CamRegs C = feature_camera(A);
    Work<false> work;
    work.clear();
    for (uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); unit < units; unit += grid_waves) {
        const uint64_t i = (uint64_t)unit * 64u + lane;
        const bool alive = i < n_pix;
        const uint32_t pi = alive ? (uint32_t)i : 0u;                       // dead lanes compute pixel 0's rays and use none of them
        const uint32_t ci = pi / A.width;
        const uint32_t x = pi - ci * A.width, y = abs_row(A, ci);

#define MIRT_FEATURE_NEAREST feature_nearest_hit_lds<GRID>(A, S, G, ro, rd, alive, closest, work, lane)
#define MIRT_FEATURE_OF_HIT feature_of_hit_lds<GRID>(A, S, best, closest, ro, rd, hn, al)
#include "mirt_feature_item_text.inc"
#undef MIRT_FEATURE_NEAREST
#undef MIRT_FEATURE_OF_HIT
    }
}

static QueryKernel feature_lds_kernel(const QueryPlan& p)
{
    return with_bools<QueryKernel>([](auto G) { return kernel_handle(feature_frame_lds_kernel<G.value>); }, p.grid);
}
