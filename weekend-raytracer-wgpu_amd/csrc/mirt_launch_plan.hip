// mirt_launch_plan.hip — the launch plan of a render call, of a query launch, and the names of their kernels (mirt_launch_plan.h): host
// arithmetic only.  The launch functions of mirt_api.hip are its callers in the library; host/plan_check.cpp calls it without a device.
#include <cstdio>

#include "mirt_kernels.h"

namespace kx = mirt::exact_build;

namespace mirt {

// ---- MirtParams row selection ----
bool rows_valid(const MirtParams* p, uint32_t* rb, uint32_t* re)
{
    const uint32_t b = p->row_begin, e = p->row_end == 0 ? p->height : p->row_end;
    if (b >= e || e > p->height) return false;
    if (p->tile_rows != 0 && p->n_parts > 1 && p->part >= p->n_parts) return false;
    *rb = b;
    *re = e;
    return true;
}

uint32_t out_rows(const MirtParams* p)
{
    uint32_t rb, re;
    if (!p || p->width == 0 || p->height == 0 || !rows_valid(p, &rb, &re)) return 0;
    const uint32_t band = re - rb;
    if (p->tile_rows == 0 || p->n_parts <= 1) return band;
    const uint32_t tr = p->tile_rows;
    const uint32_t tiles = (band + tr - 1) / tr;
    if (tiles <= p->part) return 0;
    const uint32_t owned = (tiles - p->part + p->n_parts - 1) / p->n_parts;
    uint32_t rows = owned * tr;
    if ((tiles - 1) % p->n_parts == p->part) rows -= tiles * tr - band;
    return rows;
}

MirtBvhPoolPlan plan_bvh_pool(uint32_t max_depth, bool hosek, uint64_t lds_per_cu, uint32_t only_slots, uint32_t extra_per_wave)
{
    MirtBvhPoolPlan best{};
    const uint32_t waves = kBvhPoolThreads / 64u;
    const uint64_t scene = kx::scene_lds_bytes_grid(0u, hosek);
    for (uint32_t slots : kBvhPoolSlotChoices) {
        if (only_slots != 0u && slots != only_slots) continue;
        const uint64_t block = scene + (uint64_t)waves * (bvh_pool_bytes_per_wave(slots) + extra_per_wave + 256ull * max_depth);
        uint64_t blocks = lds_per_cu / block;
        if (blocks > kBvhPoolWavesPerCu / waves) blocks = kBvhPoolWavesPerCu / waves;
        if ((uint32_t)blocks * waves > best.waves_per_cu)
            best = MirtBvhPoolPlan{ kBvhPoolThreads, slots, (uint32_t)blocks * waves, max_depth, (uint32_t)block };
        if (best.waves_per_cu == kBvhPoolWavesPerCu) break;
    }
    return best;
}

MirtBvhPoolPlan pooled_bvh_plan(const PlanFacts& f, const Tuning& tune, bool hosek, uint32_t extra_per_wave, uint32_t num_bounces)
{
    if (num_bounces > 255u) return MirtBvhPoolPlan{};
    const MirtBvhPoolPlan plan = plan_bvh_pool(f.bvh_max_depth, hosek, f.lds_per_cu, tune.hbm_pool_slots, extra_per_wave);
    return plan.slots != 0u && plan.lds_bytes_per_block <= f.lds_per_block ? plan : MirtBvhPoolPlan{};
}

MirtAdaptLdsPlan plan_adapt_lds(uint32_t n_spheres, uint32_t n_mats, uint32_t grid_bytes, bool hosek, uint64_t lds_per_cu)
{
    const uint64_t tables = grid_bytes ? (uint64_t)grid_bytes : (uint64_t)kx::scene_lds_bytes(n_spheres, n_mats, true, false) - kx::scene_lds_bytes_grid(0u, false);
    // what mirt_ctx_set_scene accepts of either layout: the budget with the sky counted, and 12-bit sphere ids in a grid
    if (kx::scene_lds_bytes_grid(0u, true) + tables > kMaxLdsBytes || (grid_bytes != 0u && n_spheres > 4095u)) return MirtAdaptLdsPlan{};
    const uint64_t block = kx::scene_lds_bytes_grid(0u, hosek) + tables;
    const uint64_t per_cu = lds_per_cu / block;
    if (per_cu == 0u) return MirtAdaptLdsPlan{};
    return MirtAdaptLdsPlan{ 256u, grid_bytes ? 1u : 0u, (uint32_t)block, (uint32_t)(per_cu < 8u ? per_cu : 8u) };
}

RenderPlan plan_render(const PlanFacts& f, const Tuning& tune, const MirtParams& p, bool frame)
{
    RenderPlan a{};
    const uint32_t rows = out_rows(&p);
    const uint64_t npix = (uint64_t)rows * p.width;
    const bool count = (p.flags & MIRT_FLAG_COUNT_WORK) != 0;
    const bool hosek = p.mode == MIRT_MODE_PT && (p.flags & MIRT_FLAG_SKY_HOSEK);

    const bool pt = p.mode == MIRT_MODE_PT;
    const size_t scene_lds = kx::scene_lds_bytes(f.n_spheres, f.n_mats, pt, hosek);
    // kernel choice (path-traced mode): the pooled kernel needs enough samples per tile to keep
    // its path pool full, 8-bit bounce counters and room for the pool beside the scene in LDS
    // MIRT_FLAG_TEXEL_TILES: flat scenes with an image texture run the pool geometry that keeps a texel window per wave
    const bool tiles = pt && (p.flags & MIRT_FLAG_TEXEL_TILES) && f.has_image_texture && tune.pool_config < 0;
    const uint32_t pool_cfg = tune.pool_config >= 0 ? (uint32_t)tune.pool_config : (tiles ? kTilePoolConfig : kDefaultPoolConfig);
    const uint32_t pool_nq = kx::pool_scatter_queues(f.n_shading_routines, count);
    const PoolConfig pc = kx::pool_config(pool_cfg, pool_nq, count);
    // Default schedule: the pooled kernel pays off when a strip holds enough samples to keep the pool full and the
    // pools still leave >= 16 waves per CU resident beside the scene tables; the sample counts from which it does are
    // measured crossovers against the strip kernel's lane-per-pixel schedule (mirt_kernels.h: kPoolMinSpp*): 28 for scenes
    // with several shading routines, 600 for single-routine scenes (nothing diverges there, so lane = pixel is hard to
    // beat: single metal sphere, 1080p x 100 spp, 1.38 ms against the pool's 1.82 and the lane-per-sample schedule's 2.27),
    // 16 for many-sphere scenes, where the pool's re-compaction of grid walks is worth most.
    const size_t lds_pool_block = scene_lds + pc.lds_bytes;
    const uint32_t pool_waves_per_cu = (uint32_t)(f.lds_per_cu / (lds_pool_block ? lds_pool_block : 1)) * (pc.threads / 64u);
    // (round 4, the streaming build of lane = pixel: a single-routine scene on a frame of at least eight rounds of 16-pixel units per resident
    //  wave -- 1 Mpixel on 256 CUs -- never takes the pool: single sphere 1080p x 800 / 2000 / 4000 spp 5.38 / 13.3 / 26.5 ms against the pool's
    //  6.34 / 15.5 / 31.2, 3840x2160 x 1000 spp 26.3 / 30.5; at 800x600 x 1000 spp the pool still wins, 2.17 against 2.31.  Scenes with several
    //  routines: streaming 1.16 ms at 32 spp, pool 1.17; 36 / 48 spp 1.28 / 1.61 against 1.24 / 1.50 -- the crossover stays.  r04_lowspp_ab.txt block 9)
    const bool stream_any_spp = f.n_shading_routines <= 1 && !hosek && npix >= 16ull * 8u * 32u * (uint64_t)f.cu_count;
    const uint32_t pool_min_spp = tune.pool_min_spp > 0 ? (uint32_t)tune.pool_min_spp
                                : stream_any_spp ? UINT32_MAX
                                : f.n_shading_routines <= 1 ? kPoolMinSppOneRoutine : kPoolMinSpp;
    bool pool = pt && p.spp >= pool_min_spp && f.n_shading_routines >= 1 && pool_waves_per_cu >= 16;
    if (p.flags & MIRT_FLAG_KERNEL_STRIP) pool = false;
    if (p.flags & MIRT_FLAG_KERNEL_POOL) pool = pt;
    // the reference's per-frame RNG stream makes a pixel's samples sequentially dependent: lane-per-pixel strip kernel only
    const bool frame_stream = pt && p.frame_spp != 0;
    if (frame_stream) pool = false;
    if (p.num_bounces > 255u || scene_lds + pc.lds_bytes > (size_t)f.lds_per_block || !f.fits_flat) pool = false;
    // Many-sphere scenes: the pool kernel's grid build keeps spheres + grid + pools in LDS (materials in L2).  It
    // is taken when the flat pool is not (too few waves per CU beside a big sphere table) and >= 12 waves fit.
    const size_t scene_lds_g = kx::scene_lds_bytes_grid(f.n_spheres, hosek);
    const bool grid_ok = pt && (!count || ((p.flags & MIRT_FLAG_COUNT_GRID) && !frame_stream)) && f.grid_bytes != 0 &&
                         !(p.flags & MIRT_FLAG_NO_GRID);
    // one 1024-thread block per CU; its path pools take what scene + grid leave of the block's LDS (counting launches:
    // the largest geometry only)
    const size_t lds_beside = scene_lds_g + f.grid_bytes;
    const size_t lds_grid_block = (size_t)f.lds_per_block / kGridPoolBlocksPerCu;
    PoolConfig pcg = kx::pool_config_grid(lds_grid_block > lds_beside ? lds_grid_block - lds_beside : 0, count);
    if (count && pcg.slots != kGridPoolSlotChoices[0] && pcg.slots != kGridPoolSlotChoices[1]) pcg.slots = 0;
    const size_t lds_pool_grid_block = lds_beside + pcg.lds_bytes;
    const uint32_t pool_grid_waves_per_cu = pcg.slots ? (uint32_t)(f.lds_per_cu / lds_pool_grid_block) * (pcg.threads / 64u) : 0u;
    bool pool_grid = grid_ok && f.grid_packable && pcg.slots != 0 && tune.pool_config < 0 && p.num_bounces <= 255u &&
                     !(p.flags & MIRT_FLAG_KERNEL_STRIP) && !frame_stream &&
                     ((p.flags & MIRT_FLAG_KERNEL_POOL) ||
                      (!pool && p.spp >= kPoolMinSppGrid && f.n_shading_routines >= 1 && pool_grid_waves_per_cu >= 16));
    if (tune.pool_grid == 0) pool_grid = false;
    if (pool_grid) pool = true;
    // MIRT_SCENE_HBM scene: the strip kernel (parity kernel) with the tables in device memory -- the BVH build unless NO_GRID asks for the
    // flat scan or a counting launch asks for the flat scan's counters (COUNT_WORK without COUNT_GRID); tile hints do not apply.
    // MIRT_FLAG_KERNEL_POOL on the BVH build: the pooled kernel (render_pt_pool_hbm_kernel) where the pool's own limits allow it -- 8-bit
    // bounce counters, no per-frame RNG stream, a geometry that fits beside the stacks of a tree this deep -- and _STRIP does not object.
    // Never by default: DESIGN.md 10.6 has the measured crossovers.
    const bool hbm = f.hbm;
    const bool hbm_bvh = hbm && pt && !(p.flags & MIRT_FLAG_NO_GRID) && (!count || (p.flags & MIRT_FLAG_COUNT_GRID));
    MirtBvhPoolPlan hbm_plan{};
    if (hbm_bvh && (p.flags & MIRT_FLAG_KERNEL_POOL) && !(p.flags & MIRT_FLAG_KERNEL_STRIP) && !frame_stream)
        hbm_plan = pooled_bvh_plan(f, tune, hosek, 0u, p.num_bounces);
    const bool pool_hbm = hbm_plan.slots != 0u;
    if (pool_hbm) pool = true;
    // the geometry of the pool kernel that will run
    // (the pooled HBM builds: the counting ones carry no register bound; no queue argument)
    const PoolConfig pcu = pool_hbm ? PoolConfig{ hbm_plan.threads, hbm_plan.slots, hbm_plan.lds_bytes_per_block, count ? 1u : kBvhPoolMinWaves, 0u }
                         : pool_grid ? pcg : pc;
    const uint32_t resident_pool_waves = pool_hbm ? hbm_plan.waves_per_cu : pool_grid ? pool_grid_waves_per_cu : pool_waves_per_cu;

    // the kernels' pinhole shortcut (generate_primary): the flag travels in the padding word beside lower_left_corner of
    // THIS launch's by-value copy of the camera; the caller's struct is never touched
    a.pinhole = (pt && tune.pinhole != 0 && f.camera_is_pinhole) ? 1u : 0u;
    a.out_rows = rows;
    a.n_units = (uint32_t)((npix + kStripPixels - 1) / kStripPixels);
    for (uint32_t l = 0; l <= kStripLevels; ++l) { a.lvl_unit[l] = a.n_units; a.lvl_pix[l] = (uint32_t)npix; }
    a.lvl_unit[0] = 0;
    a.lvl_pix[0] = 0;
    if (pool) {
        // Guided self-scheduling for the pool kernel: 16-pixel strips while more than 4 strips per resident
        // wave remain, then 8- and 4-pixel strips under the same rule, so that the waves finish within a
        // fraction of a strip of each other.  Measured on config 3 (tools/part_timing.py, one rank's share of
        // an N-way partition vs 1/N of the whole frame): fixed 16-pixel strips 95 / 83 / 67 % at N = 2 / 4 / 8,
        // this schedule 99 / 95 / 90 %; strips narrower than 4 pixels lose more to pool fill/drain than they
        // gain.  Narrow strips also need width x spp >= 512 work items to keep a wave's pool busy.
        const uint64_t waves = (uint64_t)f.cu_count * (resident_pool_waves < 32u ? resident_pool_waves : 32u);   // resident waves (LDS-bound)
        uint32_t min_width = 4;
        while (min_width < kStripPixels && (uint64_t)min_width * p.spp < 512u) min_width *= 2;
        if (tune.fixed_strips) min_width = kStripPixels;
        if (tune.gss_min_width) min_width = tune.gss_min_width;
        const double keep_factor = tune.gss_keep > 0.0 ? tune.gss_keep : 4.0;
        uint64_t pix = 0, unit = 0;
        for (uint32_t l = 0; l < kStripLevels; ++l) {
            const uint32_t width = kStripPixels >> l;
            a.lvl_unit[l] = (uint32_t)unit;
            a.lvl_pix[l] = (uint32_t)pix;
            uint64_t level_px;
            if (width <= min_width) {
                level_px = npix - pix;                               // last usable level takes the rest
            } else {
                const uint64_t keep = (uint64_t)(keep_factor * (double)(waves * width));   // pixels left for the narrower levels
                const uint64_t left = npix - pix;
                level_px = left > keep ? (left - keep) / width * width : 0;
            }
            pix += level_px;
            unit += (level_px + width - 1) / width;
        }
        a.lvl_unit[kStripLevels] = (uint32_t)unit;
        a.lvl_pix[kStripLevels] = (uint32_t)npix;
        a.n_units = (uint32_t)unit;
    }
    // many-sphere scenes: nearest hit through the uniform grid (strip kernel, non-counting build only:
    // the counting build keeps the reference's flat scan so that its work counters stay comparable)
    const bool use_grid = pool_grid || (grid_ok && !pool && scene_lds_g + f.grid_bytes + 4u * 48u <= (size_t)f.lds_per_block);
    const uint32_t grid_bytes = use_grid ? f.grid_bytes : 0u;
    a.grid_pool_slots = pool_grid ? pcg.slots : 0u;
    // camera-ray candidate lists (mirt_kernels.hip: strip_candidates): always in the pooled kernel (a list serves 16 pixels x spp rays);
    // in the strip kernel's lane-per-pixel units (64 pixels x spp) from 4 samples per pixel on -- measured on RTIOW 1080p: 2 spp +2 %
    // (selecting among 484 spheres costs more than 128 camera rays save), 8 spp -6 %
    a.strip_cand = (use_grid && tune.strip_cand != 0 && (pool_grid || p.spp >= 4u)) ? 1u : 0u;
    a.grid_flat_y = (use_grid && f.grid_flat_y) ? 1u : 0u;
    // (the strip kernel's grid build keeps a camera-ray candidate list per wave behind the blob: 4 waves x 48 bytes)
    a.lds_bytes = use_grid ? (uint32_t)(scene_lds_g + grid_bytes + (pool ? pcu.lds_bytes : 4u * 48u)) : (uint32_t)(scene_lds + (pool ? pcu.lds_bytes : 0));
    if (pool_hbm) a.lds_bytes = hbm_plan.lds_bytes_per_block;     // camera (+ sky), the block's pools, its waves' traversal stacks
    a.bvh_stack_entries = pool_hbm ? hbm_plan.stack_entries : 0u;
    if (!use_grid && !f.fits_flat && !hbm) {
        a.status = MIRT_ERR_SCENE_TOO_LARGE;
        a.message = "this scene only fits LDS in the grid build of the path-traced mode "
                    "(no parity mode, no MIRT_FLAG_COUNT_WORK / MIRT_FLAG_NO_GRID / MIRT_FLAG_KERNEL_POOL)";
        return a;
    }

    // few samples per pixel (the reference's interactive loop adds 2 per frame): lane = pixel instead of lane = sample
    // (single-routine scenes: lane = pixel at any sample count, but only for frames that give every CU a few 64-pixel units;
    //  a tiny frame with many samples per pixel needs the lanes of a wave on the samples)
    bool by_pixel = pt && !pool && !count && (p.spp < kByPixelMaxSpp || (f.n_shading_routines <= 1 && npix >= 64ull * 4u * f.cu_count));
    if (tune.by_pixel >= 0) by_pixel = pt && !pool && !count && tune.by_pixel == 1;
    if (hbm_bvh && !count && !pool_hbm) by_pixel = true;  // the BVH build's strip kernel: lane = pixel at every sample count
    if (frame_stream) by_pixel = true;                    // also for counting launches (flat scan) and any spp
    // parity mode: lane = pixel at EVERY sample count, counting or not (round 3: below 64 spp).  The reference's loop returns at the first
    // terminating sample (layer.rs:320-378), which a lane that walks its own pixel's samples does too, while lane = sample computes 64
    // samples of a pixel to find it: with one unit per wave 1080p x 64 / 100 / 1000 spp take 0.29 / 0.34 / 1.89 ms against 1.14 / 1.17 /
    // 2.08 (profiles/r04_lowspp_ab.txt block 7).  MIRT_FLAG_KERNEL_STRIP still forces lane = sample (same image, same work counters).
    if (!pt) by_pixel = (p.flags & MIRT_FLAG_KERNEL_STRIP) ? false : (tune.by_pixel >= 0 ? tune.by_pixel == 1 : true);
    a.static_units = 0;
    a.px_groups_log2 = 0;
    // lane = pixel in a flat scene from 16 spp on: the streaming build -- a lane starts its pixel's next sample without waiting for the wave
    // (mirt_kernels.hip: strip_kernel_body<STREAM>; MIRT_STREAM=0/1 for A/B runs)
    a.stream_samples = (pt && by_pixel && !count && !use_grid && p.spp >= 16u) ? 1u : 0u;
    if (tune.stream >= 0 && pt && by_pixel && !count && !use_grid) a.stream_samples = (uint32_t)tune.stream;
    if (hbm) a.stream_samples = 0u;
    if (by_pixel) {
        // Path-traced lane-per-pixel units: 64 pixels x all samples -- or 32 / 16 pixels with the samples dealt to 2 / 4 groups of lanes:
        // smaller units are more units, and the last unit of a wave is then a smaller part of its life (config 2, 1080p x 100 spp, had 4
        // units per wave: 1.21 ms; 16-pixel units, with the eight-word dispenser they need: 0.86).  Measured (tools/ab_libs.py with
        // MIRT_PX_GROUPS, profiles/r03_flat_ab.txt block 9; 1080p unless stated): as many groups as leave each >= 8 samples -- three spheres
        // at 32 / 16 / 8 spp: 1 / 2 / 4 groups 1.33 / 1.20 / 1.16, 0.68 / 0.63 / 0.66, 0.36 / 0.37 / 0.43 ms; config 2 1.17 / 0.93 / 0.86;
        // the same at 3840x2160 3.20 / 2.96 / 2.89, at 800x600 0.71 / 0.41 / 0.33 -- and one more for many-sphere scenes (RTIOW 8 spp:
        // 1.54 / 1.40).  The samples must divide evenly; never with the reference's per-frame stream (sequentially dependent samples).
        if (pt && !frame_stream && tune.px_groups != 0) {
            // (round 4, one unit per wave, profiles/r04_lowspp_ab.txt block 4: two groups from shares of 4 -- three spheres 8 spp 0.337 ms against
            //  0.359, main.rs scene 0.434 / 0.459 --, four groups from shares of 6: 16 spp 0.610 with two groups, 0.617 with four; 24 spp 0.884 / 0.881)
            // (streaming launches, below: shares of at least 8 samples -- three spheres 16 spp 0.588 ms with two groups, 0.643 with four; 24 spp
            //  0.822 / 0.886; config 2 at 25 per lane, four groups: 0.750, two: 0.829, eight (128 spp): +-0; block 9)
            const uint32_t min_share[2] = { a.stream_samples ? 8u : 4u, a.stream_samples ? 8u : (use_grid ? 4u : 6u) };
            while (a.px_groups_log2 < 2u && p.spp % (2u << a.px_groups_log2) == 0u && (p.spp >> (a.px_groups_log2 + 1u)) >= min_share[a.px_groups_log2])
                a.px_groups_log2 += 1u;
            if (tune.px_groups > 0 && p.spp % (1u << (tune.px_groups - 1)) == 0u) a.px_groups_log2 = (uint32_t)tune.px_groups - 1u;
        }
        a.n_units = (uint32_t)((npix + (64u >> a.px_groups_log2) - 1u) / (64u >> a.px_groups_log2));
        // ONE UNIT PER WAVE instead of units dispensed to a persistent grid (a.static_units; round 4): the launch has as many waves as units, and
        // the hardware's workgroup dispatcher -- which starts a block wherever a CU has room -- is the load balancer: no dispenser atomic
        // (one returning device-scope atomic per unit, 14 ns each on one address, was the whole kernel time of a 2-spp frame), and none of
        // the imbalance of dealing units round-robin to resident waves (rounds 2-3: a wave's four units are a quarter of its life each).
        // Measured against both (profiles/r04_lowspp_ab.txt block 3; 1080p, three spheres): 1 / 2 / 4 / 8 / 16 / 24 spp -14 / -16 / -13 / -4 / -2 /
        // +-0 %; main.rs scene 2 spp -20 %; config 2 -1.6 %; parity mode's lane = pixel 2 spp (1080p) -11 %, 32 spp -21 %.  Every block stages
        // the scene itself, which is why many-sphere scenes (a 25 KB grid blob per block) keep the dispenser from 4 spp on (RTIOW: 2 spp -21 %,
        // 4 / 8 / 12 spp +7 / +8 / +7 %).
        a.static_units = (!pt || !use_grid || p.spp < 4u) ? 1u : 0u;
        if (tune.static_units >= 0) a.static_units = (uint32_t)tune.static_units;
    }

    // the opt-in fast-math build of the path-traced kernels; counting launches always run the exact build
    const bool fast = pt && !count && (p.flags & MIRT_FLAG_FAST_MATH);
    a.cu_count = f.cu_count;
    a.static_grid = tune.static_grid;
    if (pool) {
        uint32_t per_cu = (uint32_t)(f.lds_per_cu / (a.lds_bytes ? a.lds_bytes : 1));
        const uint32_t by_waves = 32u / (pcu.threads / 64u);   // upper bound; LDS decides (6 blocks of 4 waves with 112-slot pools)
        if (per_cu > by_waves) per_cu = by_waves;
        if (pool_hbm) {                                        // the plan's waves, and no more blocks than the build's registers keep resident (plan_blocks)
            const uint32_t planned = hbm_plan.waves_per_cu / (pcu.threads / 64u);
            if (per_cu > planned) per_cu = planned;
        }
        if (tune.pool_blocks_per_cu >= 1 && tune.pool_blocks_per_cu < per_cu) per_cu = tune.pool_blocks_per_cu;
        a.per_cu_cap = per_cu;
        const uint32_t units_per_block = pcu.threads / 64u;
        a.blocks = (a.n_units + units_per_block - 1) / units_per_block;
    } else {
        // One unit per wave in a flat scene: one WAVE per block, too -- a block leaves when its slowest wave is done, and the scene a block
        // stages is a few hundred bytes (1080p, three spheres 2 / 4 / 8 / 16 spp -1.6 / -2.2 / -1.5 / -1.3 %, config 2 -1.9 %, parity mode at
        // 1000 spp nominal -15 %; profiles/r04_lowspp_ab.txt block 8).  Many-sphere scenes stage a 25 KB grid blob per block: 256 threads
        // (RTIOW 2 spp with 64-thread blocks: 2.4 x the time).  MIRT_STATIC_BLOCK=64/128/256 for A/B runs.
        a.launch_threads = 0u;
        if (a.static_units != 0u && tune.static_grid <= 0) a.launch_threads = tune.static_block ? tune.static_block : (use_grid ? 0u : 64u);
        const uint32_t waves_per_block = (a.launch_threads ? a.launch_threads : kBlockThreads) / 64;
        a.blocks = (a.n_units + waves_per_block - 1) / waves_per_block;
        // MIRT_SCENE_HBM: LDS holds the camera (+ sky) and, in the BVH build, every wave's traversal stacks
        if (hbm) a.lds_bytes = (uint32_t)(scene_lds_g + (hbm_bvh ? waves_per_block * kBvhStackBytesPerWave : 0u));
        a.per_cu_cap = 8u;                                            // 2048 threads per CU / 256
    }
    // kernels with dispensed units take them from eight dispenser words (mirt_kernels.hip: next_unit_any): the strip-type kernels
    // (path-traced strip kernel, both schedules; parity kernel) always.
    // The pooled kernel's strips last long at high sample counts (config 3: 9 atomics per microsecond); below 128 spp they do not
    // (three spheres, 1080p, pool forced: 48 / 64 / 100 / 200 spp -13.5 / -8.5 / -2 / +1 % with eight words; RTIOW 16 spp -4.5 %).
    a.spread_units = (a.static_units == 0u && tune.spread_units != 0 && (!pool || p.spp < 128u)) ? 1u : 0u;

    a.kernel = pool_hbm ? kKernelPtPoolHbm : hbm ? (pt ? kKernelPtHbm : kKernelParityHbm) : !pt ? kKernelParity : pool ? kKernelPtPool : kKernelPtStrip;
    a.fast = fast; a.count = count; a.hosek = hosek; a.frame = frame; a.use_grid = use_grid; a.hbm_bvh = hbm_bvh; a.by_pixel = by_pixel;
    a.stream = a.stream_samples != 0u;
    a.pool_cfg = pool_cfg; a.pool_nq = pool_nq;
    if (pool) a.pool = pcu;
    return a;
}

void plan_blocks(RenderPlan& a, uint32_t resident_per_cu)
{
    const bool pool = a.kernel == kKernelPtPool || a.kernel == kKernelPtPoolHbm;
    uint32_t blocks = a.blocks;
    if (pool) {
        uint32_t per_cu = a.per_cu_cap;
        if (resident_per_cu >= 1u && per_cu > resident_per_cu) per_cu = resident_per_cu;
        if (per_cu == 0u) per_cu = 1u;
        if (blocks > a.cu_count * per_cu) blocks = a.cu_count * per_cu;
    } else {
        // a persistent grid of exactly the blocks that are resident at once: registers and LDS decide (4-8 per CU for these
        // kernels).  A block beyond that would hold its first unit until the dispenser has run dry and run it alone at the end.
        const uint32_t per_cu = resident_per_cu > a.per_cu_cap ? a.per_cu_cap : resident_per_cu;
        const uint32_t resident = a.cu_count * per_cu;
        // ... unless the launch runs one unit per wave (a.static_units): then the grid is the units (MIRT_STATIC_GRID=k, A/B runs: k x the
        // resident blocks with the units dealt round-robin, rounds 2-3's schedule at k = 1)
        uint32_t cap = resident;
        if (a.static_units != 0u) cap = a.static_grid > 0 ? resident * (uint32_t)a.static_grid : blocks;
        if (blocks > cap) blocks = cap;
    }
    if (blocks == 0) blocks = 1;
    a.blocks = blocks;

    // the dispenser continues after the units the waves take by their own index (first_unit() in the kernels)
    const uint32_t launched_waves = blocks * ((pool ? a.pool.threads : (a.launch_threads ? a.launch_threads : kBlockThreads)) / 64u);
    a.first_dispensed = launched_waves;          // the words themselves are zero (retire_slots): no memset node in front of the kernel
    for (uint32_t x = 0; x < 8u; ++x) a.disp_taken[x] = launched_waves > x ? (launched_waves - x + 7u) / 8u : 0u;
}

void plan_kernel_name(const RenderPlan& pl, char* out, size_t n)
{
    const char* const tf[2] = { "false", "true" };
    const char* const fast = pl.fast ? "fast_build::" : "", *const kframe = pl.frame ? "_frame" : "";
    const char* const count = tf[pl.count], *const hosek = tf[pl.hosek];
    const PoolConfig& g = pl.pool;
    switch (pl.kernel) {
    case kKernelParity:    snprintf(out, n, "render_parity_kernel<%s,%s>", count, tf[pl.by_pixel]); break;
    case kKernelParityHbm: snprintf(out, n, "render_parity_hbm_kernel<%s,%s>", count, tf[pl.by_pixel]); break;
    case kKernelPtStrip:   // (a counting grid build is lane = sample whatever by_pixel says: render_kernel)
        if (pl.stream) snprintf(out, n, "%srender_pt_stream%s_kernel<%s>", fast, kframe, hosek);
        else snprintf(out, n, "%srender_pt_strip%s_kernel<%s,%s,%s,%s>", fast, kframe, count, hosek, tf[pl.use_grid], tf[pl.by_pixel && !(pl.count && pl.use_grid)]);
        break;
    case kKernelPtHbm:     // (the non-counting BVH build is lane = pixel whatever by_pixel says)
        snprintf(out, n, "%srender_pt_hbm%s_kernel<%s,%s,%s,%s>", fast, kframe, count, hosek, tf[pl.hbm_bvh], tf[pl.by_pixel || (pl.hbm_bvh && !pl.count)]);
        break;
    case kKernelPtPoolHbm: snprintf(out, n, "%srender_pt_pool_hbm%s_kernel<%u,%u,%u,%s,%s>", fast, kframe, g.threads, g.slots, g.min_waves, count, hosek); break;
    case kKernelPtPool:    // <threads, slots, min waves, COUNT, HOSEK, NQ, GRID, FLATY>; the tile build's name has always stopped at GRID
        if (!pl.use_grid && pl.pool_cfg == kTilePoolConfig)
            snprintf(out, n, "%srender_pt_pool_tile%s_kernel<%u,%u,%u,%s,%s,%u,false>", fast, kframe, g.threads, g.slots, g.min_waves, count, hosek, g.queues);
        else
            snprintf(out, n, "%srender_pt_pool%s_kernel<%u,%u,%u,%s,%s,%u,%s,%s>", fast, kframe, g.threads, g.slots, g.min_waves, count, hosek, g.queues, tf[pl.use_grid],
                     tf[pl.use_grid && pl.grid_flat_y != 0u]);
        break;
    }
}

// ---- query launches ----
// The tree and the traversal stacks of the query kernels that run one thread per ray or pixel in kBlockThreads blocks (ray queries, feature
// frames): the stacks hold as many node references per lane as the resident tree is deep (a push happens at inner nodes only, at
// most one per level): 256 x depth bytes per wave, as in the pooled kernel -- at most 32 KB per block (MIRT_BVH_MAX_DEPTH)
static QueryPlan plan_block_query(const PlanFacts& f, QueryFamily family, bool bvh, uint64_t items)
{
    QueryPlan a{};
    a.family = family; a.bvh = bvh; a.threads = kBlockThreads;
    a.bvh_stack_entries = bvh ? (f.bvh_max_depth ? f.bvh_max_depth : 1u) : 0u;
    a.lds_bytes = (kBlockThreads / 64u) * 64u * 4u * a.bvh_stack_entries;
    a.blocks = (uint32_t)((items + kBlockThreads - 1u) / kBlockThreads);
    return a;
}

// The layout of an MIRT_ADAPT_LDS step or an MIRT_QUERY_LDS query on the resident LDS scene: the scene's grid unless
// `flat` asks for the flat scan (MIRT_FLAG_NO_GRID; a query family's _FLAT bit), else the flat tables if they fit; plan_adapt_lds's geometry of
// it, or all fields 0 where neither fits a block's LDS.
static MirtAdaptLdsPlan adapt_lds_layout(const PlanFacts& f, bool flat, bool hosek)
{
    MirtAdaptLdsPlan plan{};
    if (f.grid_bytes != 0u && !flat) plan = plan_adapt_lds(f.n_spheres, f.n_mats, f.grid_bytes, hosek, f.lds_per_cu);
    if (plan.lds_bytes_per_block > f.lds_per_block) plan = MirtAdaptLdsPlan{};
    if (plan.threads == 0u && f.fits_flat) plan = plan_adapt_lds(f.n_spheres, f.n_mats, 0u, hosek, f.lds_per_cu);
    if (plan.lds_bytes_per_block > f.lds_per_block) plan = MirtAdaptLdsPlan{};
    return plan;
}

// An MIRT_QUERY_LDS query over `items` rays or pixels: the family's LDS kernel in the layout's geometry, a persistent grid before its
// occupancy cap (query_plan_blocks), or the refusal a render with MIRT_FLAG_NO_GRID gives on a grid-only scene.
static QueryPlan plan_lds_query(const PlanFacts& f, const Tuning& tune, QueryFamily family, bool flat, bool hosek, uint64_t items)
{
    QueryPlan a{};
    const MirtAdaptLdsPlan lds = adapt_lds_layout(f, flat, hosek);
    a.family = family; a.hosek = hosek; a.grid = lds.grid != 0u;
    if (lds.threads == 0u) {
        a.status = MIRT_ERR_SCENE_TOO_LARGE;
        a.message = flat ? "this scene fits LDS in neither layout an MIRT_QUERY_LDS query has (the _FLAT bit: the flat one only)"
                         : "this scene fits LDS in neither layout an MIRT_QUERY_LDS query has";
        return a;
    }
    a.threads = kQueryLdsThreads; a.lds_bytes = lds.lds_bytes_per_block;
    a.blocks = (uint32_t)((items + kQueryLdsThreads - 1u) / kQueryLdsThreads);
    a.cu_count = f.cu_count; a.blocks_per_cu = lds.blocks_per_cu; a.at_most_blocks = tune.query_lds_blocks;
    return a;
}

QueryPlan plan_trace(const PlanFacts& f, const Tuning& tune, uint32_t n_rays, uint32_t flags)
{
    if (!f.hbm && (flags & MIRT_QUERY_LDS)) {      // the schedule hint MIRT_RAYS_SORT is accepted and ignored: no tree to take bounds from
        QueryPlan a = plan_lds_query(f, tune, kQueryTraceLds, (flags & MIRT_RAYS_FLAT) != 0, false, n_rays);
        a.any = (flags & MIRT_RAYS_ANY_HIT) != 0; a.count = (flags & MIRT_RAYS_COUNT) != 0;
        a.n_rays = n_rays;
        return a;
    }
    QueryPlan a = plan_block_query(f, kQueryTrace, !(flags & MIRT_RAYS_FLAT), n_rays);
    a.any = (flags & MIRT_RAYS_ANY_HIT) != 0; a.count = (flags & MIRT_RAYS_COUNT) != 0; a.sorted = (flags & MIRT_RAYS_SORT) != 0;
    a.n_rays = n_rays;
    return a;
}

QueryPlan plan_features(const PlanFacts& f, const Tuning& tune, const MirtParams& p, uint32_t flags)
{
    if (!f.hbm && (flags & MIRT_QUERY_LDS)) return plan_lds_query(f, tune, kQueryFeaturesLds, (flags & MIRT_FEATURES_FLAT) != 0, false, (uint64_t)out_rows(&p) * p.width);
    return plan_block_query(f, kQueryFeatures, !(flags & MIRT_FEATURES_FLAT), (uint64_t)out_rows(&p) * p.width);
}

// What the radiance query and the adaptive step share.  Unpooled: `items` rays or pixels, one per thread, one wave per block; path_radiance
// walks the tree as the strip kernels do, with a stack of MIRT_BVH_MAX_DEPTH entries per lane behind the staged camera (+ sky).
// Pooled (`pool` has slots): units of 16 items, one unit per wave -- the hardware's dispatcher is the balancer --; `at_most` != 0
// (MIRT_*_POOL_BLOCKS): no more blocks than that, their waves stride over the units.  LDS: camera words (+ sky), the block's pools, its
// waves' traversal stacks.
static QueryPlan plan_path_query(const PlanFacts& f, QueryFamily unpooled, QueryFamily pooled, bool bvh, bool hosek, uint64_t items, uint32_t wave_threads,
                                 const MirtBvhPoolPlan& pool, uint32_t at_most)
{
    QueryPlan a{};
    a.bvh = bvh; a.hosek = hosek;
    if (pool.slots == 0u) {
        a.family = unpooled; a.threads = wave_threads;
        a.lds_bytes = (uint32_t)(kx::scene_lds_bytes_grid(f.n_spheres, hosek) + (bvh ? kBvhStackBytesPerWave : 0u));
        a.n_units = (uint32_t)items;
        a.blocks = (uint32_t)(((uint64_t)a.n_units + wave_threads - 1u) / wave_threads);
        return a;
    }
    a.family = pooled;
    a.threads = pool.threads; a.slots = pool.slots; a.min_waves = kBvhPoolMinWaves;
    a.lds_bytes = pool.lds_bytes_per_block; a.bvh_stack_entries = pool.stack_entries;
    const uint64_t units = (items + kStripPixels - 1u) / kStripPixels, waves = pool.threads / 64u, blocks = (units + waves - 1u) / waves;
    a.n_units = (uint32_t)units;
    a.blocks = (uint32_t)(at_most != 0u && blocks > at_most ? at_most : blocks);
    return a;
}

QueryPlan plan_radiance(const PlanFacts& f, const Tuning& tune, uint32_t n_rays, const MirtRadianceParams& p)
{
    const bool bvh = !(p.flags & MIRT_RADIANCE_FLAT), hosek = (p.flags & MIRT_RADIANCE_SKY_HOSEK) != 0;
    if (!f.hbm && (p.flags & MIRT_QUERY_LDS)) {    // the schedule hints MIRT_RADIANCE_SORT and _POOL are accepted and ignored: no tree, no pooled LDS query build
        QueryPlan a = plan_lds_query(f, tune, kQueryRadianceLds, !bvh, hosek, n_rays);
        a.n_units = n_rays; a.n_rays = n_rays;
        return a;
    }
    MirtBvhPoolPlan pool{};
    if ((p.flags & MIRT_RADIANCE_POOL) && bvh) pool = pooled_bvh_plan(f, tune, hosek, 0u, p.num_bounces);
    QueryPlan a = plan_path_query(f, kQueryRadiance, kQueryRadiancePool, bvh, hosek, n_rays, kRadianceThreads, pool, tune.radiance_pool_blocks);
    a.sorted = (p.flags & MIRT_RADIANCE_SORT) != 0;
    a.rays_as_row = a.family == kQueryRadiancePool;       // its units are slots of the batch: the kernel reads the batch's length where a render reads the width
    a.n_rays = n_rays;
    return a;
}

QueryPlan plan_adapt(const PlanFacts& f, const Tuning& tune, const MirtParams& q, uint32_t adapt_flags, bool run, uint64_t buffer_pixels)
{
    const bool hosek = (q.flags & MIRT_FLAG_SKY_HOSEK) != 0;
    QueryPlan a{};
    if (!f.hbm) {
        // a scene that lives in LDS (the caller has seen MIRT_ADAPT_LDS): adapt_pixels_lds_kernel over the staged scene of the layout
        const MirtAdaptLdsPlan lds = adapt_lds_layout(f, (q.flags & MIRT_FLAG_NO_GRID) != 0, hosek);
        a.family = kQueryAdaptLds;
        a.hosek = hosek; a.grid = lds.grid != 0u;
        if (lds.threads == 0u) {
            a.status = MIRT_ERR_SCENE_TOO_LARGE;
            a.message = (q.flags & MIRT_FLAG_NO_GRID) ? "this scene fits LDS in neither layout an MIRT_ADAPT_LDS step has (MIRT_FLAG_NO_GRID: the flat one only)"
                                                      : "this scene fits LDS in neither layout an MIRT_ADAPT_LDS step has";
            return a;
        }
        a.threads = lds.threads; a.lds_bytes = lds.lds_bytes_per_block;
        a.n_units = (uint32_t)buffer_pixels; a.px_groups_log2 = tune.adapt_lds_groups;
        a.blocks = (uint32_t)((buffer_pixels + lds.threads - 1u) / lds.threads);
        a.cu_count = f.cu_count; a.blocks_per_cu = lds.blocks_per_cu; a.at_most_blocks = tune.adapt_lds_blocks;
    } else {
        // MIRT_ADAPT_POOL on the BVH build: adapt_pixels_pool_kernel in the geometry mirt_adapt_pool_plan gives for the resident tree
        const bool bvh = !(q.flags & MIRT_FLAG_NO_GRID);
        MirtBvhPoolPlan pool{};
        if ((adapt_flags & MIRT_ADAPT_POOL) && bvh) pool = pooled_bvh_plan(f, tune, hosek, kAdaptPoolExtraBytes, q.num_bounces);
        a = plan_path_query(f, kQueryAdapt, kQueryAdaptPool, bvh, hosek, buffer_pixels, kAdaptThreads, pool, tune.adapt_pool_blocks);
        // (the host does not know the step's count: either grid is for all pixels, n_units the buffer's in both)
        a.n_units = (uint32_t)buffer_pixels;
    }
    a.run = run;
    return a;
}

void query_plan_blocks(QueryPlan& a, uint32_t resident_per_cu)
{
    if (!query_family_lds(a.family)) return;
    uint32_t per_cu = resident_per_cu;
    if (per_cu > a.blocks_per_cu) per_cu = a.blocks_per_cu;
    if (per_cu == 0u) per_cu = 1u;
    const uint64_t resident = (uint64_t)a.cu_count * per_cu;
    if (a.blocks > resident) a.blocks = (uint32_t)resident;
    if (a.at_most_blocks != 0u && a.blocks > a.at_most_blocks) a.blocks = a.at_most_blocks;
}

void query_kernel_name(const QueryPlan& pl, char* out, size_t n)
{
    const char* const tf[2] = { "false", "true" };
    const char* const sorted = pl.sorted ? "_sorted" : "", *const run = pl.run ? "_run" : "", *const hosek = tf[pl.hosek];
    switch (pl.family) {
    case kQueryTrace:        snprintf(out, n, "trace_rays%s_kernel<%s,%s,%s>", sorted, tf[pl.bvh], tf[pl.any], tf[pl.count]); break;
    case kQueryFeatures:     snprintf(out, n, "feature_frame_kernel<%s>", tf[pl.bvh]); break;
    case kQueryRadiance:     snprintf(out, n, "radiance_rays%s_kernel<%s,%s>", sorted, hosek, tf[pl.bvh]); break;
    case kQueryRadiancePool: snprintf(out, n, "radiance_rays_pool_kernel<%u,%u,%u,%s,%s>", pl.threads, pl.slots, pl.min_waves, hosek, tf[pl.sorted]); break;
    case kQueryAdapt:        snprintf(out, n, "adapt_pixels%s_kernel<%s,%s>", run, hosek, tf[pl.bvh]); break;
    case kQueryAdaptPool:    snprintf(out, n, "adapt_pixels_pool%s_kernel<%u,%u,%u,%s>", run, pl.threads, pl.slots, pl.min_waves, hosek); break;
    case kQueryAdaptLds:     snprintf(out, n, "adapt_pixels_lds%s_kernel<%s,%s>", run, hosek, tf[pl.grid]); break;
    case kQueryTraceLds:     snprintf(out, n, "trace_rays_lds_kernel<%s,%s,%s>", tf[pl.grid], tf[pl.any], tf[pl.count]); break;
    case kQueryFeaturesLds:  snprintf(out, n, "feature_frame_lds_kernel<%s>", tf[pl.grid]); break;
    case kQueryRadianceLds:  snprintf(out, n, "radiance_rays_lds_kernel<%s,%s>", hosek, tf[pl.grid]); break;
    }
}

}  // namespace mirt
