// mirt_launch_plan.h — the launch plan of a render call: which kernel runs, in which geometry and with which schedule, as plain
// data computed by two pure functions, and a third that prints the kernel's name (mirt_launch_plan.hip); below it the same for the query
// launches (QueryPlan).  No HIP call, no context, no getenv, no allocation: host arithmetic over a handful of numbers, so that a machine
// without a GPU can check it (host/plan_check.cpp, tests/test_launch_plan.py, tests/test_launch_kernels.py, tests/test_query_plan.py).
// Plain C++ on top of include/mirt.h: g++ compiles it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/mirt.h"

namespace mirt {

constexpr uint32_t kStripLevels   = 5;    // strip widths 16, 8, 4, 2, 1
constexpr uint32_t kStripPixels   = 16;   // strip kernels: pixels one wave owns per work unit (64-B RGBA8 store)
constexpr uint32_t kBlockThreads  = 256;  // strip kernels: 4 waves
constexpr uint32_t kByPixelMaxSpp = 64;   // strip kernel: below this many samples per pixel a wave takes 64 pixels, lane = pixel (scenes with
                                          // one shading routine: at any sample count -- nothing diverges, 1.51 ms against 2.27 on config 2)
// Samples per pixel from which the pooled kernel is the default (below: the strip kernel, lane = pixel).  A 16-pixel strip
// of few samples cannot keep a pool full (about 25 steps of fill and drain per strip whatever it holds), so the thresholds are
// measured crossovers (tools/ab_libs.py with MIRT_FLAG_KERNEL_STRIP / _POOL, 1080p):
//   several shading routines (config 3): strip 1.58 / 1.73 / 1.94 ms at 36 / 40 / 44 spp, pool 1.61 / 1.67 / 1.74   -> 40 (round 2)
//     round 3 (sample groups; eight-word dispenser in both kernels): strip 0.98 / 1.13 / 1.24 / 1.37 / 1.54 ms at 24 / 28 / 32 / 36 / 40 spp, pool
//     1.00 / 1.11 / 1.21 / 1.30 / 1.41 (main.rs 5-sphere scene: 1.32 / 1.65 against 1.33 / 1.55 at 24 / 32 spp)                                   -> 28
//   ONE routine (config 2, no divergence for the lane-per-pixel kernel to lose): round 2 184; round 3: strip 0.93 / 1.78 / 3.55 / 5.21 / 6.98 /
//     8.48 ms at 100 / 200 / 400 / 600 / 800 / 1000 spp, pool 1.81 / 2.42 / 3.85 / 5.17 / 6.52 / 7.96                                           -> 600
//   many-sphere scenes (grid build, RTIOW): round 2: strip 2.09 / 4.11 / 7.69 ms at 8 / 16 / 32 spp, pool 2.31 / 3.14 / 4.66 -> 16;
//     round 3: strip 1.54 / 2.19 / 2.70 ms at 8 / 12 / 16 spp, pool 1.99 / 2.28 / 2.61                                                          -> 16
//   round 4 (lane-per-pixel launches run one unit per wave; profiles/r04_lowspp_ab.txt block 5): several routines: strip 0.96 / 1.10 / 1.27 /
//     1.52 ms at 24 / 28 / 32 / 40 spp, pool 1.01 / 1.12 / 1.20 / 1.39 (main.rs scene 1.26 / 1.66 against 1.32 / 1.56 at 24 / 32)             -> 32
//     ONE routine: strip 3.36 / 4.81 / 6.49 / 8.11 ms at 400 / 600 / 800 / 1000 spp, pool 3.80 / 5.25 / 6.52 / 7.93                           -> 800
//     with the streaming build of lane = pixel (from 16 spp on; block 9): several routines: 0.94 / 1.16 / 1.28 / 1.61 ms at 28 / 32 / 36 / 48 spp, pool
//     - / 1.17 / 1.24 / 1.50                                                                                                                  -> 32
//     ONE routine: 5.38 / 13.3 / 26.5 ms at 800 / 2000 / 4000 spp, pool 6.34 / 15.5 / 31.2; 3840x2160 x 1000 spp 26.3 against 30.5 -> frames of
//     >= 1 Mpixel never take the pool (mirt_launch_plan.hip: stream_any_spp); 800x600 x 1000 spp 2.31 against the pool's 2.17                  -> 800 below that
constexpr uint32_t kPoolMinSpp           = 32;
constexpr uint32_t kPoolMinSppOneRoutine = 800;
constexpr uint32_t kPoolMinSppGrid       = 16;

// The geometry of a pool kernel's build, which is every number among its template arguments: threads per block, path slots per wave, the
// waves per SIMD it is held to (launch bounds) and its scatter queues (0: pooled HBM, which has no such argument); and the LDS of a block's pools.
struct PoolConfig { uint32_t threads, slots, lds_bytes, min_waves, queues; };

// Tuning / experiment knobs.  They are read from the environment ONCE, when a context is created
// (mirt_ctx_create), never inside a render call: a shipped library must not change its schedule
// because a variable appeared mid-run, and getenv has no place in a sub-millisecond launch path.
struct Tuning {
    int      pool_config = -1;        // MIRT_POOL_CONFIG: geometry of the path pool (index into kPoolConfigs)
    int      pool_grid = -1;          // MIRT_POOL_GRID=0: never take the pool kernel's grid build
    bool     fixed_strips = false;    // MIRT_STRIP_MODE=16: fixed 16-pixel strips (no guided self-scheduling)
    uint32_t gss_min_width = 0;       // MIRT_GSS_MINW: narrowest strip of the guided schedule
    double   gss_keep = 0.0;          // MIRT_GSS_KEEP: strips per resident wave kept for the narrower levels
    int      by_pixel = -1;           // MIRT_BY_PIXEL=0/1: force lane = sample / lane = pixel in the strip kernel
    uint32_t pool_blocks_per_cu = 0;  // MIRT_POOL_BLOCKS_PER_CU: fewer resident pool blocks (occupancy experiments)
    double   grid_cell = 0.0;         // MIRT_GRID_CELL: cell size of the uniform grid in median radii
    double   grid_big = 0.0;          // MIRT_GRID_BIG: spheres above this many median radii stay outside the grid
    int      pinhole = -1;            // MIRT_PINHOLE=0: never take the pinhole-camera shortcut (A/B runs)
    int      spread_units = -1;       // MIRT_SPREAD_UNITS=0: strip-type launches use one dispenser word (A/B runs)
    int      static_units = -1;       // MIRT_STATIC_UNITS=0/1: lane-per-pixel units dispensed to a persistent grid / one unit per wave (A/B runs, tests)
    int      pool_min_spp = -1;       // MIRT_POOL_MIN_SPP=n: flat scenes take the pooled kernel from n samples per pixel on (A/B runs: the crossovers kPoolMinSpp*)
    int      stream = -1;             // MIRT_STREAM=0/1: lane-per-pixel launches in flat scenes never / always run the streaming build (A/B runs)
    int      px_groups = -1;          // MIRT_PX_GROUPS=0: lane-per-pixel units are always 64 pixels; 1 / 2 / 3: force 1 / 2 / 4 sample groups (A/B runs)
    int      strip_cand = -1;         // MIRT_STRIP_CAND=0: camera rays of grid builds take the grid like every other ray (A/B runs)
    int      grid_flat_y = -1;        // MIRT_GRID_FLAT_Y=0: a grid one cell high is walked in three dimensions like any other (A/B runs, tests)
    bool     debug_slots = false;     // MIRT_DEBUG_SLOTS=1: every launch checks (synchronously) that its slot's dispenser words are zero
    uint32_t static_block = 0;        // MIRT_STATIC_BLOCK=64/128/256 (A/B runs): threads per block of the launches that run one unit per wave
    int      static_grid = -1;        // MIRT_STATIC_GRID=k (A/B runs): launches with one unit per wave run k x the resident blocks instead, units dealt round-robin
    int      timing = -1;             // MIRT_TIMING=0/1: the context's initial mirt_ctx_set_timing state (A/B runs; default 1)
    uint32_t hbm_pool_slots = 0;      // MIRT_HBM_POOL_SLOTS=n (A/B runs): the pooled build of MIRT_SCENE_HBM scenes takes this one of kBvhPoolSlotChoices
    uint32_t radiance_pool_blocks = 0;    // MIRT_RADIANCE_POOL_BLOCKS=n (A/B runs, tests): a pooled radiance query launches at most n blocks, whose waves stride over the units
    uint32_t adapt_pool_blocks = 0;   // MIRT_ADAPT_POOL_BLOCKS=n (A/B runs, tests): a pooled adaptive step launches at most n blocks, whose waves stride over the units
    uint32_t adapt_lds_blocks = 0;    // MIRT_ADAPT_LDS_BLOCKS=n (A/B runs, tests): an MIRT_ADAPT_LDS step launches at most n blocks
    uint32_t query_lds_blocks = 0;    // MIRT_QUERY_LDS_BLOCKS=n (A/B runs, tests): an MIRT_QUERY_LDS launch (ray, feature or radiance query on a scene in LDS) launches at most n blocks
    int32_t  denoise_staged = -1;     // MIRT_DENOISE_STAGED=mask (A/B runs, tests): bit i set: level i of mirt_ctx_denoise* runs the staged shape; -1: the measured choice
    uint32_t adapt_lds_groups = 0;    // MIRT_ADAPT_LDS_GROUPS=1/2/3 (A/B runs, tests): an MIRT_ADAPT_LDS step deals samples to 1 / 2 / 4 groups of lanes (capped by spp)
    bool     ext_events = true;       // MIRT_EXT_EVENTS=0: the event pair as two records in the stream instead of riding on the kernel dispatch (A/B runs)
};

// What the planner reads of a context, and nothing more.
struct PlanFacts {
    uint32_t cu_count;                            // device
    uint64_t lds_per_cu, lds_per_block;
    uint32_t n_spheres, n_mats, n_shading_routines;   // scene
    bool     has_image_texture, have_sky, fits_flat, hbm;
    uint32_t grid_bytes;                          // grid (0: the scene has none)
    bool     grid_packable, grid_flat_y, have_shade;
    uint32_t bvh_max_depth;                       // tree of a MIRT_SCENE_HBM scene
    bool     camera_is_pinhole;                   // camera
};

// The kernel a plan runs.  Together with the bits below it names one template instance: render_kernel(plan) of the plan's build
// (mirt_kernels.h) is that instance -- what the occupancy question is asked of and what is dispatched (mirt_api.hip) --, and
// plan_kernel_name(plan) prints it for mirt_ctx_last_kernel.  Both read the plan and nothing else.
enum PlanKernel : uint32_t { kKernelParity, kKernelParityHbm, kKernelPtStrip, kKernelPtHbm, kKernelPtPool, kKernelPtPoolHbm };

struct RenderPlan {
    int         status;               // MIRT_OK, or the one refusal (MIRT_ERR_SCENE_TOO_LARGE) with its message
    const char* message;
    // the kernel
    PlanKernel kernel;
    bool       fast, count, hosek, frame, use_grid, hbm_bvh, by_pixel, stream;
    uint32_t   pool_cfg, pool_nq;
    PoolConfig pool;                  // geometry of the pool kernel that runs (zero for the other kernels)
    // the schedule (the RenderArgs fields of the same names)
    uint32_t out_rows, n_units, lvl_unit[kStripLevels + 1], lvl_pix[kStripLevels + 1];
    uint32_t px_groups_log2, static_units, stream_samples, strip_cand, grid_flat_y, grid_pool_slots;
    uint32_t launch_threads, lds_bytes, bvh_stack_entries, spread_units;
    uint32_t pinhole;                 // the word that travels in the camera's padding (generate_primary's shortcut)
    uint32_t blocks;                  // plan_render: before the occupancy cap; plan_blocks: the grid of the launch
    // what plan_blocks needs besides the occupancy answer, and what it adds
    uint32_t cu_count, per_cu_cap;    // blocks per CU at most: LDS, waves, the pooled HBM plan, MIRT_POOL_BLOCKS_PER_CU (pool kernels); 8 (strip-type)
    int      static_grid;             // Tuning.static_grid
    uint32_t first_dispensed, disp_taken[8];
};

// The geometry of the pooled kernel of MIRT_SCENE_HBM scenes (mirt_bvh_pool_plan; the launch calls this very function) for a tree
// `max_depth` deep: per block the camera (+ sky), and per wave a pool and 64 stacks of max_depth entries.  The rule (mirt_kernels.h,
// DESIGN.md 10.6): the first of kBvhPoolSlotChoices -- largest pools first -- that leaves kBvhPoolWavesPerCu waves resident, else the
// choice with most waves, the larger pools on a tie.  slots == 0: not even one block fits.  `only_slots` != 0 (A/B runs): that choice alone.
// `extra_per_wave`: bytes a wave keeps beside its pool -- 0 for the pooled render and the pooled query, kAdaptPoolExtraBytes for the
// pooled adaptive step (mirt_adapt_pool_plan).
MirtBvhPoolPlan plan_bvh_pool(uint32_t max_depth, bool hosek, uint64_t lds_per_cu, uint32_t only_slots, uint32_t extra_per_wave);

// The gate every pooled BVH launch passes (render, radiance query, adaptive step): 8-bit bounce counters, and a geometry for the
// resident tree that fits the block's LDS.  slots == 0: none, the launch is the one without the pool.
MirtBvhPoolPlan pooled_bvh_plan(const PlanFacts& f, const Tuning& tune, bool hosek, uint32_t extra_per_wave, uint32_t num_bounces);

// The geometry of an MIRT_ADAPT_LDS step (mirt_adapt_lds_plan; the launch calls this very function): 256-thread blocks that
// stage camera (+ sky) and either the grid blob (grid_bytes != 0) or the sphere and material tables, at most 8 of them per CU.  All fields
// 0: a layout the render launches refuse (mirt_ctx_set_scene's budget, which counts the sky; a grid over more than 4 095 spheres), or
// not even one block per CU.
MirtAdaptLdsPlan plan_adapt_lds(uint32_t n_spheres, uint32_t n_mats, uint32_t grid_bytes, bool hosek, uint64_t lds_per_cu);

// MirtParams row selection: is it valid (then [*rb, *re) is the band), and the rows a call writes (mirt_params_out_rows)
bool     rows_valid(const MirtParams* p, uint32_t* rb, uint32_t* re);
uint32_t out_rows(const MirtParams* p);

// Everything a render launch decides before it asks for occupancy: kernel, geometry, schedule.  `frame`: a progressive frame (sums AND image).
RenderPlan plan_render(const PlanFacts& f, const Tuning& tune, const MirtParams& p, bool frame);
// The caps that need the occupancy answer -- blocks of the chosen kernel resident per CU (0: no answer) --, then the dispenser's start.
void plan_blocks(RenderPlan& plan, uint32_t resident_per_cu);
// The name mirt_ctx_last_kernel reports: the plan's kernel template and its arguments, without spaces, as the tests and tools read them;
// "fast_build::" in front of the fast-math build's.
void plan_kernel_name(const RenderPlan& plan, char* out, size_t out_len);

// ---- query launches: ray queries, feature frames, radiance queries, adaptive steps and runs ----
constexpr uint32_t kRadianceThreads = 64;    // radiance_rays_kernel: one wave per block (mirt_radiance_kernel.inc has the measurement)
constexpr uint32_t kAdaptThreads    = 64;    // adapt_pixels_kernel: one wave per block, as kRadianceThreads
constexpr uint32_t kAdaptLdsThreads = 256;   // adapt_pixels_lds_kernel: four waves share one staged scene
constexpr uint32_t kQueryLdsThreads = 256;   // trace_rays_lds_kernel, feature_frame_lds_kernel, radiance_rays_lds_kernel: the same shape

// The kernel family of a query launch; with the bits below it names one template instance of the exact build: query_kernel(plan)
// (mirt_kernels.h) is that instance and query_kernel_name(plan) prints it for mirt_ctx_last_kernel.
//   trace          trace_rays[_sorted]_kernel<bvh, any, count>                      one thread per ray, kBlockThreads
//   features       feature_frame_kernel<bvh>                                        one thread per pixel, kBlockThreads
//   radiance       radiance_rays[_sorted]_kernel<hosek, bvh>                        one thread per ray, one wave per block
//   radiance-pool  radiance_rays_pool_kernel<threads, slots, min waves, hosek, sorted>   units of 16 rays, one per wave, or the waves stride
//   adapt          adapt_pixels[_run]_kernel<hosek, bvh>                            one thread per pixel of the buffer, one wave per block
//   adapt-pool     adapt_pixels_pool[_run]_kernel<threads, slots, min waves, hosek>  units of 16 pixels of the buffer, as radiance-pool
//   adapt-lds      adapt_pixels_lds[_run]_kernel<hosek, grid>                       a persistent grid of the blocks resident at once
//   trace-lds      trace_rays_lds_kernel<grid, any, count>                          MIRT_QUERY_LDS on a scene in LDS: adapt-lds's shape,
//   features-lds   feature_frame_lds_kernel<grid>                                   units of 64 consecutive rays or pixels, lane = ray or pixel
//   radiance-lds   radiance_rays_lds_kernel<hosek, grid>
enum QueryFamily : uint32_t { kQueryTrace, kQueryFeatures, kQueryRadiance, kQueryRadiancePool, kQueryAdapt, kQueryAdaptPool, kQueryAdaptLds,
                              kQueryTraceLds, kQueryFeaturesLds, kQueryRadianceLds };
constexpr bool query_family_lds(QueryFamily f) { return f == kQueryAdaptLds || f == kQueryTraceLds || f == kQueryFeaturesLds || f == kQueryRadianceLds; }

// What a query launch decides, and the contract between it and its kernel: fill_query_args (mirt_api.hip) copies the fields of the
// second group into RenderArgs beside what every launch carries (fill_common_args), launch_query dispatches `blocks` x `threads`.
struct QueryPlan {
    int         status;               // MIRT_OK, or the one refusal (the LDS families: MIRT_ERR_SCENE_TOO_LARGE, no layout fits a block's LDS) with its message
    const char* message;
    // the kernel
    QueryFamily family;
    bool        bvh, any, count, sorted, hosek, grid, run;
    uint32_t    threads, slots, min_waves;   // threads per block of the launch; pooled families: with slots and min waves the build's template arguments
    // RenderArgs
    uint32_t    lds_bytes;            // trace, features: the block's traversal stacks, 256 bytes x bvh_stack_entries per wave; radiance, adapt: the staged camera
                                      // (+ sky) and, walking the tree, the wave's kBvhStackBytesPerWave; pooled: plan_bvh_pool's block; adapt-lds: plan_adapt_lds's
    uint32_t    bvh_stack_entries;    // trace, features: the depth of the resident tree (at least 1), 0 for the flat scan; pooled: the tree's depth; else 0 =
                                      // MIRT_BVH_MAX_DEPTH, the strip kernels' stacks.  adapt-lds has no tree: its launch leaves every bvh_* field zero
    uint32_t    n_units;              // radiance, radiance-lds: rays; radiance-pool: units of 16 rays; adapt families: pixels of the buffer; else 0
    uint32_t    px_groups_log2;       // adapt-lds: 0 (the device chooses) or the forced g + 1 (Tuning.adapt_lds_groups); else 0
    bool        rays_as_row;          // radiance-pool: RenderArgs.width = n_rays, height = 1.  (`grid`: grid, grid_bytes, grid_flat_y travel; the LDS families: sph3 too)
    uint32_t    n_rays;               // trace: the kernel's own argument behind the buffers; radiance(-pool): the batch's length
    uint32_t    blocks;               // the grid of the launch; the LDS families: before the occupancy cap (query_plan_blocks)
    uint32_t    cu_count, blocks_per_cu, at_most_blocks;     // the LDS families, for query_plan_blocks: the layout's own bound (plan_adapt_lds), Tuning.adapt_lds_blocks / query_lds_blocks
};

// flags: the caller's MIRT_RAYS_* / MIRT_FEATURES_* bits; adapt_flags: MirtAdaptParams.flags; n_rays > 0; `p`, `rows` (= out_rows(&p)): the
// params of a feature frame as checked; `q`: those of an adaptive step as check_adapt_step leaves them; `run`: a step of a run (planned
// once per call); buffer_pixels: records in the context's adaptive buffer.  A pooled request that pooled_bvh_plan gives no geometry
// plans the launch without the pool.  MIRT_QUERY_LDS in the flags of a ray, feature or radiance query on a scene that lives in LDS (!f.hbm; the
// caller has checked the flag) plans the family's LDS kernel over plan_adapt_lds's geometry of the layout: the scene's grid unless the family's
// _FLAT bit is set, else the flat tables if they fit, else MIRT_ERR_SCENE_TOO_LARGE.  An HBM scene ignores the flag.
QueryPlan plan_trace(const PlanFacts& f, const Tuning& tune, uint32_t n_rays, uint32_t flags);
QueryPlan plan_features(const PlanFacts& f, const Tuning& tune, const MirtParams& p, uint32_t flags);
QueryPlan plan_radiance(const PlanFacts& f, const Tuning& tune, uint32_t n_rays, const MirtRadianceParams& p);
QueryPlan plan_adapt(const PlanFacts& f, const Tuning& tune, const MirtParams& q, uint32_t adapt_flags, bool run, uint64_t buffer_pixels);
// The LDS families (query_family_lds), shaped like plan_blocks: a persistent grid of the blocks resident at once -- the smaller of the occupancy answer and the layout's
// bound, at least one per CU --, or fewer for fewer items or Tuning.adapt_lds_blocks / query_lds_blocks; the other families' grids need no answer: nothing
void query_plan_blocks(QueryPlan& plan, uint32_t resident_per_cu);
// The name mirt_ctx_last_kernel reports, written as plan_kernel_name writes a render kernel's
void query_kernel_name(const QueryPlan& plan, char* out, size_t out_len);

}  // namespace mirt
