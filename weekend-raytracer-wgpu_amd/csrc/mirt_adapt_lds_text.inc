// mirt_adapt_lds_text.inc -- the render stage of an adaptive step on a scene that lives in LDS (MIRT_ADAPT_LDS; DESIGN.md 10.15), as TEXT:
// mirt_adapt_lds_kernel.inc includes it twice.
//   MIRT_ADAPT_LDS_KERNEL   the kernel's name: adapt_pixels_lds_kernel (a step) or adapt_pixels_lds_run_kernel (a step of a run)
//   MIRT_ADAPT_RUN          0: a pixel's sample count is the launch's, A.spp
//                           1: it is the word behind the count (head[1], which adapt_scan_run_kernel wrote for this step), read as a
//                              wave-uniform word next to the count, before anything is staged (DESIGN.md 10.14)
// GRID: the scene's uniform grid (camera (+ sky) | blob in LDS, a hit's sphere and material from device memory), else the flat layout
// (camera | spheres | materials (| sky) in LDS), exactly what the strip kernel's lane-per-pixel builds stage.
// A.px_groups_log2: 0 = the rule of mirt_adapt_rule.h chooses g; k > 0 = g is k - 1 (MIRT_ADAPT_LDS_GROUPS), still capped by spp.
template <bool HOSEK, bool GRID>
__global__ __launch_bounds__(kAdaptLdsThreads, kAdaptLdsMinWaves) void MIRT_ADAPT_LDS_KERNEL(RenderArgs A, adapt_u4* recs, const uint32_t* list, const uint32_t* count_word)
{
    const uint32_t count = __builtin_amdgcn_readfirstlane(*count_word);
#if MIRT_ADAPT_RUN
    const uint32_t spp = __builtin_amdgcn_readfirstlane(count_word[1]);      // 0 exactly when count is 0
#else
    const uint32_t spp = A.spp;
#endif
    constexpr uint32_t kWaves = kAdaptLdsThreads / 64u;
    const uint32_t grid_waves = gridDim.x * kWaves;
    uint32_t g = adapt_lds_groups(count, spp, grid_waves);
    if (A.px_groups_log2 != 0u) {                                      // a forced g, held to the shares spp allows (and to 0 for an empty list)
        const uint32_t g_cap = adapt_lds_groups(count, spp, 0xffffffffu);
        g = A.px_groups_log2 - 1u < g_cap ? A.px_groups_log2 - 1u : g_cap;
    }
    const uint32_t unit_px = 64u >> g;
    const uint32_t units = count / unit_px + (count % unit_px != 0u ? 1u : 0u);      // <= 2^30
#define MIRT_LDS_SKY HOSEK
#include "mirt_lds_block_text.inc"
#undef MIRT_LDS_SKY
    const uint32_t grp = lane >> (6u - g);                             // which share of the samples this lane takes
    const uint32_t n_mine = spp >> g;                                  // wave-uniform: 1 << g divides spp
    Work<false> work;
    work.clear();
    for (uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); unit < units; unit += grid_waves) {
        const uint64_t slot = (uint64_t)unit * unit_px + (lane & (unit_px - 1u));
        const bool alive = slot < count;
        const uint64_t pi = alive ? list[slot] : 0u;                   // the record's place in the band; < out_rows x width (adapt_compact_kernel)
        const uint32_t ci = (uint32_t)pi / A.width;
        const uint32_t x = (uint32_t)pi - ci * A.width;
        const uint32_t y = abs_row(A, ci);
        const uint32_t n = alive ? recs[4u * pi + 3u].x : 0u;          // every group reads the pixel's sample count
        const uint32_t s_first = n + grp * n_mine;
        unsigned long long sum_r = 0, sum_g = 0, sum_b = 0, even_r = 0, even_g = 0, even_b = 0;
        for (uint32_t j = 0; j < n_mine; ++j) {
            Rng rng;
            f3 ro, rd;
            {   // camera constants are re-read from LDS per sample instead of living in 21 VGPRs (strip_kernel_body)
                const CamRegs C = load_camera(S, A);
                generate_primary(A, C, x, y, s_first + j, rng, ro, rd);
            }
            const f3 c = path_radiance<false, HOSEK, GRID, kSrcLds>(A, S, G, alive, rng, ro, rd, work, lane, nullptr, kNoCand, nullptr);
            const unsigned long long fr = to_fixed(c.x), fg = to_fixed(c.y), fb = to_fixed(c.z);
            sum_r += fr; sum_g += fg; sum_b += fb;
            if (((s_first + j) & 1u) == 0u) { even_r += fr; even_g += fg; even_b += fb; }
        }
        for (uint32_t off = unit_px; off < 64u; off <<= 1) {           // add the shares: lanes l, l + unit_px, ... hold one pixel
            sum_r += __shfl_xor(sum_r, (int)off, 64); sum_g += __shfl_xor(sum_g, (int)off, 64); sum_b += __shfl_xor(sum_b, (int)off, 64);
            even_r += __shfl_xor(even_r, (int)off, 64); even_g += __shfl_xor(even_g, (int)off, 64); even_b += __shfl_xor(even_b, (int)off, 64);
        }
        if (alive && grp == 0u) {                                      // the record is read only now: its sums are no registers of the sample loop
            const adapt_u4 q0 = recs[4u * pi], q1 = recs[4u * pi + 1u], q2 = recs[4u * pi + 2u];
            sum_r += adapt_u64(q0.x, q0.y); sum_g += adapt_u64(q0.z, q0.w); sum_b += adapt_u64(q1.x, q1.y);
            even_r += adapt_u64(q1.z, q1.w); even_g += adapt_u64(q2.x, q2.y); even_b += adapt_u64(q2.z, q2.w);
            recs[4u * pi] = adapt_u4{ (uint32_t)sum_r, (uint32_t)(sum_r >> 32), (uint32_t)sum_g, (uint32_t)(sum_g >> 32) };
            recs[4u * pi + 1u] = adapt_u4{ (uint32_t)sum_b, (uint32_t)(sum_b >> 32), (uint32_t)even_r, (uint32_t)(even_r >> 32) };
            recs[4u * pi + 2u] = adapt_u4{ (uint32_t)even_g, (uint32_t)(even_g >> 32), (uint32_t)even_b, (uint32_t)(even_b >> 32) };
            recs[4u * pi + 3u] = adapt_u4{ n + spp, 0u, 0u, 0u };
        }
    }
}
