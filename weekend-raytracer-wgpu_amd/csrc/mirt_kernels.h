// mirt_kernels.h — launch interface between the C ABI (mirt_api.hip) and the gfx950 kernels
// (mirt_kernels.hip).  Plain structs, passed by value as kernel arguments.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirt.h"
#include "mirt_launch_plan.h"     // PoolConfig, the strip constants and the pool thresholds: what the launch plan shares with the kernels

namespace mirt {

// A sphere as the kernels read it from LDS: the reference's 32-byte `Sphere`
// (src/raytracer/mod.rs:418-431) with its two padding words replaced by values every
// intersection needs.  rr = radius*radius and inv_r = 1.0f/radius are computed once on the host
// in IEEE binary32 — the same roundings the per-test expressions `sphere.radius * sphere.radius`
// (mod.rs:1135, wgsl:411) and `1.0 / radius` (mod.rs:1233, wgsl:433) produce.
struct PreparedSphere {
    float    cx, cy, cz, rr;
    float    inv_r, radius;
    uint32_t material_idx;
    uint32_t op;            // pool kernel: queue of its material's shading routine (RenderArgs.queue_routine)
};
static_assert(sizeof(PreparedSphere) == 32, "PreparedSphere must stay 2 x 16 B for ds_read_b128");

// A material as the path-traced kernels read it from LDS: `GpuMaterial` (mod.rs:757-765) plus
// values derived once on the host: 1/x (the dielectric's `1f / refractionIndex`, wgsl:261) and,
// for 1x1 textures (every colour material of the reference's scenes), the texel itself so that
// the common lookup needs no global-memory access.
//   tex[k] for a 1x1 texture: { r, g, b, bits(offset) };  otherwise { bits(w), bits(h), bits(offset), 0 }.
struct PreparedMaterial {
    uint32_t id;
    float    x;
    float    inv_x;
    uint32_t flags;            // bit 0: desc1 is 1x1, bit 1: desc2 is 1x1
    float    tex[2][4];
};
static_assert(sizeof(PreparedMaterial) == 48, "PreparedMaterial is 3 x 16 B");

// Many-sphere scenes (grid builds): what shading a hit on sphere i needs besides what the grid blob already holds in LDS (centre,
// routine id): 1/r and the sphere's material, in ONE 64-byte line of global memory -- no sphere -> material_idx -> material chain.
// The scatter step loads `a` and `t0` (two independent 16-byte loads; `t1` only in the checkerboard's case) and uses them after
// the routine's random draws (mirt_kernels.hip: shade_grid_hit).
struct ShadeRec {
    float a[4];        // {1/r, x, 1/x, bits(flags)}
    float t0[4];       // first texture (PreparedMaterial.tex[0])
    float t1[4];       // second texture (checkerboard only)
    float c[4];        // {centre, bits(id)}: not read by the kernels (centre and routine id come from the grid blob in LDS)
};
static_assert(sizeof(ShadeRec) == 64, "ShadeRec is one 64-byte line");

// Uniform grid over the small spheres of a many-sphere scene (>= kGridMinSpheres): the nearest-hit scan
// visits only the cells a ray crosses (3D-DDA) plus a short list of "big" spheres.  The grid is
// CONSERVATIVE (every sphere is listed in all cells its enlarged bounding box touches; the enlargement covers the rounding of
// the walk and, for ray origins within GridHeader.guard, of the sphere test -- mirt_kernels.hip above GridLds) and the
// hit rule breaks ties by sphere index, so the result is identical to the reference's flat scan.
// Layout of the blob (all of it is staged into LDS; the kernels of a grid build read NO other sphere data from LDS):
//   GridHeader | big ids [n_big] u16 | FURTHER item ids [n_items] u16 (a cell's third, fourth ... sphere, ascending)
//   | routine of every sphere [n_spheres] u8 = min(GpuMaterial.id, 4): what a scatter step switches on
//   | 8-byte aligned: cell table [ncells] of two u32 = {first further item | item count << 16, id0 | id1 << 16}: the first two sphere ids
//     of a cell arrive WITH its entry, so their records are one LDS round trip away (entry -> records) instead of two (entry -> ids ->
//     records) -- most cells list at most two spheres (RTIOW: 0.84 tests per visited cell) -- round 4, -2 % on RTIOW
//   | 16-byte aligned: test records {cx, cy, cz, r^2} of the big spheres [n_big], in list order (a COPY: the always-tested list
//     needs no id -> record indirection) | of EVERY sphere [n_spheres], by sphere id.
// A record is the first half of the sphere's PreparedSphere.  (Round 2 stored a record per list ENTRY -- a sphere listed in k cells stored
// k times, 17 KB for RTIOW; stored once per sphere the cells can be made smaller without the blob outgrowing LDS: cell = 2.5 median radii
// instead of 4, -9 % on RTIOW.)
struct GridHeader {
    float    org[3];        // lower corner
    float    cell[3];       // cell size per axis
    float    inv_cell[3];
    uint32_t dims[3];
    uint32_t n_big;         // spheres tested for every ray (too large for the grid)
    uint32_t off_big;       // offsets in uint16 units from the start of the blob
    uint32_t off_cells;     // BYTE offset (multiple of 4) of the cell table
    uint32_t off_items;     // sphere ids, ascending within a cell
    uint32_t total_bytes;   // multiple of 16
    uint32_t off_ops;       // BYTE offset of the per-sphere routine-queue table
    uint32_t off_big_recs;  // BYTE offsets (multiples of 16) of the test records: the big spheres' copies ...
    uint32_t off_recs;      // ... and every sphere's, by id
    uint32_t n_entries;     // cell entries in total (a sphere counts once per cell that lists it)
    float    inv_dim_x;     // 1 / dims[0] and 1 / (dims[0] * dims[1]), IEEE quotients from the host: a parked walk's linear cell index is
    float    inv_dim_xy;    // taken apart with them (floor((n + 0.5) * inv) == n / d exactly for n, d <= 8192: tests/test_abi.py)
    uint32_t n_spheres;     // records behind off_recs (the far-origin scan of the strip kernels, see `guard`)
    // The far-origin guard (mirt_kernels.hip: "what the binning absorbs").  The binning enlargement covers the rounding of the sphere
    // test only for rays whose origin lies within `L_safe - R_g` of the centre C_g of a sphere (C_g, R_g) around every binned sphere:
    // guard = {C_g, (L_safe / 1.02 - R_g)^2, or -1 when that difference is not positive}; a ray with |o - C_g|^2 above guard[3]
    // (or NaN) does not trust the walk.  bound_r = R_g.
    float    guard[4];
    float    bound_r;
    uint32_t pad_[3];
};
static_assert(sizeof(GridHeader) % 16 == 0, "GridHeader is staged with 16-byte copies");
#ifndef MIRT_DISPENSER_STRIDE
#define MIRT_DISPENSER_STRIDE 1024           // u32 words between a launch's eight dispenser words: 4 KB, so that they sit in different memory channels
#endif
constexpr uint32_t kGridMinSpheres = 32;
constexpr uint32_t kGridMaxCells   = 4096;   // x 8 bytes per cell entry = the 32 KB of LDS that round 3's 8 192 four-byte entries could take: the pools keep their room
                                            // (a soup of 700 small spheres over a wide volume lost every pool geometry to a 64 KB cell table: soak seed 3150)

#if defined(MIRT_DIAG_STEPS) || defined(MIRT_DIAG_STAMPS)   // diagnosis builds (tools/step_stats.py): ten more counters, printed by mirt_ctx_get_stats
constexpr uint32_t kNumCounters   = 31;
#else
constexpr uint32_t kNumCounters   = 18;   // u64 work counters (MirtStats order)
#endif
constexpr uint32_t kMaxLdsBytes   = 120 * 1024; // scene budget in LDS (of 160 KB per CU); sphere ids are 12 bit in the pool kernel

// pooled path-traced kernel: every wave keeps a pool of paths in LDS, queued by pending shading routine
constexpr uint32_t kDefaultPoolConfig = 0;
// MIRT_FLAG_TEXEL_TILES: the pool geometry with an LDS texel window per wave (render_pt_pool_tile_kernel)
#ifndef MIRT_TILE_SLOTS
#define MIRT_TILE_SLOTS 112
#endif
constexpr uint32_t kTilePoolConfig = 5, kTilePoolSlots = MIRT_TILE_SLOTS;
// pool kernel, grid build (many-sphere scenes): ONE 1024-thread block per CU, so that the grid blob (~20 KB for RTIOW)
// is staged once for all 16 waves and the rest of the 160 KB goes to the path pools.  Measured on RTIOW 1080p x 128 spp:
// 512 threads x 112 slots, two blocks 17.3 ms; x 128 slots 16.6; 1024 x 144 15.9; 1024 x 152 15.7; one 512-thread
// block per CU (8 waves) with 160-256 slots 26.3 -- the pools want to be as large as 16 resident waves allow.
// 160 slots are the first choice where a small blob leaves room for them (they cost nothing there); on RTIOW a blob shrunk until they
// fit measured +-0 against 152 (profiles/r04_c5_ab.txt block 4), which is why plan_grid coarsens cells only until 152 fit, not 160.
// (experiment builds: -DMIRT_GRID_THREADS=640 -DMIRT_GRID_BLOCKS=2 -DMIRT_GRID_MINW=5 "-DMIRT_GRID_SLOTS=104,96,88,80" = 20 waves per CU)
#ifndef MIRT_GRID_THREADS
#define MIRT_GRID_THREADS 1024
#define MIRT_GRID_BLOCKS 1
#define MIRT_GRID_MINW 4
#define MIRT_GRID_SLOTS 160, 152, 128, 96
#endif
constexpr uint32_t kGridPoolThreads = MIRT_GRID_THREADS;
constexpr uint32_t kGridPoolBlocksPerCu = MIRT_GRID_BLOCKS;    // blocks of the grid build that share a CU's LDS
constexpr uint32_t kGridPoolMinWaves = MIRT_GRID_MINW;         // waves per SIMD the build is held to (launch bounds)
constexpr uint32_t kGridPoolSlotChoices[4] = { MIRT_GRID_SLOTS };   // the largest geometry whose block fits LDS is taken

enum CounterSlot : uint32_t {
    kCntRays = 0, kCntTests, kCntRoots, kCntHits,
    kCntScatter0, kCntScatter1, kCntScatter2, kCntScatter3, kCntScatter4,
    kCntSky, kCntLaneIters, kCntWaveIters,
    kCntCells, kCntWaveCells,           // grid builds: cells visited by lanes / cell-loop iterations of waves
    kCntTexelsPrimary, kCntTileHitsPrimary,   // tile build: image-texel fetches of camera-ray hits / of those, served by the LDS tile
    kCntTexelsLater, kCntTileHitsLater        // ... of later bounces
};

struct RenderArgs {
    // The camera travels BY VALUE with every launch (96 B of kernel arguments, staged into LDS from the kernarg
    // segment): `Layer::update_camera` / `set_render_params` (layer.rs:188-193, mod.rs:353-388) change it every
    // interactive frame, and this way mirt_ctx_set_camera needs no device copy and no synchronisation, and a
    // launch already queued keeps the camera it was issued with.  MUST stay the first member (stage_scene).
    MirtGpuCamera           cam;
    const PreparedSphere*   spheres;
    const MirtMaterial*     mats;          // reference layout (parity kernel)
    const PreparedMaterial* pmats;         // derived layout (path-traced kernels)
    const float*            texels;
    const MirtSkyState*     sky;
    uint32_t*               out;           // compact RGBA8, one u32 per pixel
    unsigned long long*     counters;      // [kNumCounters] of THIS launch (one block per event slot), COUNT builds only
    const unsigned char*    grid;          // nullable: GridHeader + lists (strip kernel, GRID build)
    const ShadeRec*         shade;         // grid builds: [n_spheres] shading records (nullable otherwise)
    uint32_t                grid_bytes;
    uint32_t                grid_pool_slots;   // pool kernel, grid build: slots per wave of the geometry chosen on the host
    uint32_t                strip_cand;        // pool kernel, grid build: 1 = camera rays scan their strip's candidate list (0: A/B runs)
    uint32_t                grid_flat_y;       // grid builds: 1 = the grid is ONE cell high (dims[1] == 1: spheres on a ground plane) -> the 2-D walk
    uint32_t*               work_counter;  // dynamic work dispenser: THIS launch's own word (one per event slot), preset before the launch
    unsigned long long*     accum;         // nullable: [pixels][3] exact fixed-point sums to ADD into instead of resolving; with `out` set too, a
                                           // progressive frame (the *_frame_kernel builds): add, and write the resolve of the updated sums to `out`
    uint64_t                n_texels;
    uint32_t n_spheres, n_mats;
    uint32_t width, height, spp, num_bounces, flags, seed_mix, sample_begin;
    uint32_t frame_begin;                  // frames before this accumulation (MirtParams.frame_begin)
    uint32_t frame_spp;                    // > 0: the reference's per-frame RNG stream (MirtParams.frame_spp); lane-per-pixel schedule
    uint32_t row_begin, tile_rows, n_parts, part;
    uint32_t out_rows;                     // rows this launch writes
    uint32_t n_units;                      // work units (strips) the dispenser hands out
    uint32_t first_dispensed;              // the dispenser's words start at ZERO (pre-zeroed per launch slot, no memset node in front of the kernel):
                                           // units below this one -- one per launched wave -- are taken by wave index (first_unit)
    uint32_t disp_taken[8];                // eight-word dispenser: how many of word x's units (u = 8 k + x) those are
    uint32_t static_units;                 // lane-per-pixel kernels: no dispenser -- unit = wave index (+ the grid's waves, if the host launched fewer waves than units)
    uint32_t spread_units;                 // strip-type kernels: units from eight dispenser words (unit u <-> word u mod 8; next_unit_any)
    uint32_t px_groups_log2;               // lane-per-pixel strip kernel: a unit is 64 >> g pixels, their samples dealt to 1 << g groups of lanes
    // pool kernel, guided self-scheduling: level l = strips of (kStripPixels >> l) pixels; it starts at unit
    // lvl_unit[l] / pixel lvl_pix[l] (entry kStripLevels = end).  Strips shrink 16 -> 1 pixels towards the end of
    // the frame so that all waves finish within a fraction of a strip of each other.
    uint32_t lvl_unit[6];
    uint32_t lvl_pix[6];
    uint32_t queue_routine[5];             // pool kernel: scatter queue q runs routine queue_routine[q] = min(GpuMaterial.id, 4)
    uint32_t lds_bytes;
    uint32_t launch_threads;               // strip-type kernels: threads per block of THIS launch (0: kBlockThreads)
    uint32_t stream_samples;               // lane-per-pixel strip launch in a flat scene: 1 = render_pt_stream_kernel (a lane starts its next sample without waiting for the wave)
    float    sph3[12];                     // scenes of exactly three spheres: their {centre, r^2} records as kernel arguments (scalar loads)
    // MIRT_SCENE_HBM scenes, BVH build of render_pt_hbm_kernel (mirt_bvh.h; appended so that no older field moves)
    const float4*   bvh_nodes;             // [n_nodes] BvhNode, four float4 each
    const float4*   bvh_recs;              // {centre, r^2}: the always-tested list [bvh_n_always], then the leaves' spheres
    const uint32_t* bvh_ids;               // original sphere index of every record
    uint32_t        bvh_root;              // reference of the root (BvhNode child encoding)
    uint32_t        bvh_n_always;
    float           bvh_centre[3];         // a sphere around every tree sphere's box, and the largest |radius| in the tree:
    float           bvh_radius, bvh_rmax;  // the traversal's rounding bound (nearest_hit_bvh)
    uint32_t        bvh_stack_entries;     // render_pt_pool_hbm_kernel: node references per lane of a wave's traversal stacks = the depth of the
                                           // resident tree (MirtBvhInfo.plan.max_depth); the strip builds always keep MIRT_BVH_MAX_DEPTH
};
// MIRT_SCENE_HBM, BVH build: every wave keeps 64 per-lane traversal stacks of MIRT_BVH_MAX_DEPTH node references in LDS
constexpr uint32_t kBvhStackBytesPerWave = 64u * MIRT_BVH_MAX_DEPTH * 4u;

// MIRT_SCENE_HBM, pooled build (render_pt_pool_hbm_kernel, MIRT_FLAG_KERNEL_POOL): 256-thread blocks whose waves keep a
// two-queue pool (WavePoolLayout<SLOTS, 1>: 50 x SLOTS + 384 bytes) and, behind the block's pools, 64 traversal stacks of as many
// entries as the resident tree is deep (256 x depth bytes per wave).  The geometry is chosen per launch by plan_bvh_pool (mirt_launch_plan.hip,
// mirt_bvh_pool_plan): the largest pools that leave kBvhPoolWavesPerCu waves resident, or, where no choice does, the choice that keeps
// most waves (the larger pools on a tie).  The non-counting builds are held to the registers of that many waves.
constexpr uint32_t kBvhPoolThreads = 256;
constexpr uint32_t kBvhPoolMinWaves = 4;                          // waves per SIMD (launch bounds): 16 per CU
constexpr uint32_t kBvhPoolWavesPerCu = 4u * kBvhPoolMinWaves;
constexpr uint32_t kBvhPoolSlotChoices[4] = { 112, 96, 80, 64 };
constexpr uint32_t bvh_pool_bytes_per_wave(uint32_t slots) { return 50u * slots + 384u; }     // == WavePoolLayout<slots, 1>::kBytes (static_assert in the kernel)
// The pooled adaptive step (adapt_pixels_pool_kernel, MIRT_ADAPT_POOL) keeps behind that pool the 16 x 3 `even` accumulators
// (384 bytes) and the {place in the band, samples so far} of its 16 list entries (128 bytes): mirt_adapt_pool_plan's bytes per wave
constexpr uint32_t kAdaptPoolExtraBytes = 512;
constexpr uint32_t adapt_pool_bytes_per_wave(uint32_t slots) { return bvh_pool_bytes_per_wave(slots) + kAdaptPoolExtraBytes; }     // (static_assert in the kernel)

// The parts of a tile-interleaved frame and where they go (assemble_parts_kernel).  Two forms:
//   table  (part_stride_px == 0): parts[i] is part i's compact buffer, n_parts <= kAssembleMaxParts (the node's members);
//   stride (part_stride_px != 0): part i starts at parts[0] + i * part_stride_px, any n_parts (mirt_ctx_deinterleave_device).
// vec4 = 1 only if every row start is 16-byte aligned: width % 4 == 0, the part pointers (or base and stride) and out 16-byte aligned.
constexpr uint32_t kAssembleMaxParts = 16;
struct AssembleArgs {
    const uint32_t* parts[kAssembleMaxParts];
    uint32_t*       out;        // band image [band_rows][width]
    uint64_t        part_stride_px;
    uint32_t        width, band_rows, tile_rows, n_parts;
    uint32_t        vec4;
};

// Where a render kernel is dispatched: the stream, and optionally the event pair of the launch.  Non-null events ride on the kernel
// dispatch itself (hipExtLaunchKernel attaches start / stop timestamps to the dispatch) instead of two event-record packets in the stream.
struct LaunchOn {
    hipStream_t stream = nullptr;
    hipEvent_t  begin = nullptr, end = nullptr;
    LaunchOn(hipStream_t s = nullptr, hipEvent_t b = nullptr, hipEvent_t e = nullptr) : stream(s), begin(b), end(e) {}
};

// launchers (mirt_kernels.hip).  That file is compiled twice: namespace exact_build (the default, bit-exact arithmetic;
// everything below) and namespace fast_build (mirt_kernels_fast.hip: MIRT_FLAG_FAST_MATH, hardware transcendentals;
// the path-traced render kernels only).
// render_kernel: the one template instance a launch plan names -- of all six PlanKernel families, from the plan's bits alone --, or nullptr
// where the build has none (parity mode and every counting launch in fast_build).  mirt_ctx_last_kernel reports the same instance
// (plan_kernel_name, mirt_launch_plan.h).
using RenderKernel = void (*)(RenderArgs);
using QueryKernel = const void*;      // a query kernel's handle: what the runtime's launch, attribute and occupancy calls take
struct QueryBuffers { const void* in; void* out; const uint32_t* order; const uint32_t* count; };
namespace fast_build {
RenderKernel render_kernel(const RenderPlan& plan);
}
namespace exact_build {
RenderKernel render_kernel(const RenderPlan& plan);
// kernel<<<blocks, threads, a.lds_bytes, on>>>(a), for the kernels of either build
hipError_t launch_with_lds(RenderKernel kernel, uint32_t blocks, uint32_t threads, const RenderArgs& a, LaunchOn on);
// blocks of `kernel` that are resident per CU at once (hipOccupancyMaxActiveBlocksPerMultiprocessor), asked once per kernel and LDS size
uint32_t   blocks_per_cu(RenderKernel kernel, uint32_t threads, uint32_t lds_bytes);
uint32_t   pool_config_count();
// the geometry of the pool build that runs: flat geometry i for a scene of nq shading queues ...
PoolConfig pool_config(uint32_t i, uint32_t nq, bool count);
// ... and the grid build's: slots by the LDS left beside scene + grid (slots = 0: none fits)
PoolConfig pool_config_grid(size_t lds_for_pools, bool count);
uint32_t pool_scatter_queues(uint32_t n_routines, bool count);
hipError_t launch_resolve(const unsigned long long* accum, uint32_t* out, uint64_t n_pixels, uint32_t n_samples,
                          uint32_t flags, hipStream_t stream);
hipError_t launch_selftest_math(unsigned long long* d_mismatches, hipStream_t stream);
// d_counts[3]: decided inputs, parity mismatches and zeros among them (mirt_ctx_selftest_checker_sign)
hipError_t launch_selftest_checker_sign(unsigned long long* d_counts, hipStream_t stream);
// The query launches (ray queries, feature frames, radiance queries, the render stage of an adaptive step): query_kernel is the one template
// instance a QueryPlan names (mirt_launch_plan.h, which also says what `a` must carry), nullptr where there is none; launch_query dispatches
// it in the plan's geometry with `a` and the family's buffers, all in device memory:
//   trace                 in: [n_rays] MirtRay, out: [n_rays] MirtRayHit, 4-byte aligned; order: the permutation of a sorted launch, [n_rays] words
//   features              out: [out_rows x width] MirtFeaturePixel, 4-byte aligned
//   radiance(-pool)       in: [n_rays] MirtRadianceRay, out: [n_rays] MirtRadiance, 4-byte aligned; order: as above (nullptr: the caller's order)
//   adapt(-pool, -lds)    out: the buffer's MirtAdaptPixel records, 16-byte aligned; order: the step's list; count: its head words {count, a run's spp}
QueryKernel query_kernel(const QueryPlan& plan);
hipError_t  launch_query(const QueryPlan& plan, const RenderArgs& a, const QueryBuffers& b, hipStream_t stream);
uint32_t    blocks_per_cu(QueryKernel kernel, uint32_t threads, uint32_t lds_bytes);        // as above, of a query kernel
// mirt_ctx_adapt_* (mirt_adapt_kernel.inc).  The select stage of a step over n >= 1 records (MirtAdaptPixel, 16-byte aligned):
// adapt_select_kernel, adapt_scan_kernel, adapt_compact_kernel -- d_flags [n] bytes, d_block_counts [ceil(n / 256)] words, d_list [n] words, d_head
// four words {count of the step, unused, 64-bit counter of samples added (+= count x spp)}, 8-byte aligned.
hipError_t launch_adapt_select(const void* d_recs, uint32_t n, const MirtAdaptParams& adapt, uint32_t spp, unsigned char* d_flags, uint32_t* d_block_counts,
                               uint32_t* d_list, uint32_t* d_head, hipStream_t stream);
// The select stage of a step of a RUN (mirt_ctx_adapt_run_device): adapt_scan_run_kernel in the middle, whose thread 0 chooses the
// step's sample count on the device -- adapt_run_spp(count, base_spp, min_items, cap_spp) of mirt_adapt_rule.h -- writes it to d_head[1], adds
// count x that to the counter and writes {count, spp} to d_log_entry (8-byte aligned).
hipError_t launch_adapt_select_run(const void* d_recs, uint32_t n, const MirtAdaptParams& adapt, uint32_t base_spp, uint32_t min_items, uint32_t cap_spp,
                                   unsigned char* d_flags, uint32_t* d_block_counts, uint32_t* d_list, uint32_t* d_head, void* d_log_entry, hipStream_t stream);
// adapt_resolve_kernel: n_pixels records -> RGBA8, every pixel over its own sample count
hipError_t launch_adapt_resolve(const void* d_recs, uint32_t* out, uint64_t n_pixels, uint32_t flags, hipStream_t stream);
// mirt_ctx_denoise* (mirt_denoise_kernel.inc): denoise_prepare_kernel<source> and `levels` launches of denoise_atrous_kernel, the last
// with its epilogue (RGBA8 per `flags`, or float32).  d_src: the accumulation sums (n_samples for every pixel) or the MirtAdaptPixel records;
// d_guides: [width x rows] MirtFeaturePixel, 4-byte aligned; inv[levels]: every level's 1 / sg^2; d_scratch: three planes of 16 bytes per pixel;
// bit i of staged_levels: level i runs denoise_atrous_staged_kernel.
hipError_t launch_denoise(uint32_t source, const void* d_src, uint32_t n_samples, const void* d_guides, uint32_t width, uint32_t rows, uint32_t levels,
                          uint32_t normal_log2, bool colour, const float* inv, bool f32_out, uint32_t flags, uint32_t staged_levels, void* d_scratch, void* d_out,
                          hipStream_t stream);
// mirt_ctx_reproject* (mirt_reproject_kernel.inc): reproject_kernel<clamp, rgba8> over a band of width x rows pixels that starts at
// image row row_begin.  All six planes hold the compact band, 4-byte aligned; d_rgba8 null: no RGBA8 plane.  `flags`: the two tone flags.
struct ReprojectArgs {
    MirtGpuCamera previous, current;
    uint32_t width, height, row_begin, rows;
    uint32_t flags;
    float    max_history, depth_tolerance;
    uint32_t tiles_x;              // ceil(width / 64); a tile is 64 x 4 pixels
    uint64_t tiles;
};
hipError_t launch_reproject(ReprojectArgs a, bool clamp, const void* d_colour, const void* d_guides, const void* d_prev_colour, const void* d_prev_guides,
                            void* d_out, void* d_rgba8, hipStream_t stream);
hipError_t launch_assemble(const AssembleArgs& a, LaunchOn on);
size_t     scene_lds_bytes(uint32_t n_spheres, uint32_t n_mats, bool pt, bool hosek);
size_t     scene_lds_bytes_grid(uint32_t n_spheres, bool hosek);
}  // namespace exact_build

// host side (mirt_api.hip): sets the thread's mirt_last_error() message and returns `status`
int set_error(int status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// host side (mirt_api.hip): would mirt_ctx_accum_frame_device accept these params on this context now (the output apart)?  MIRT_OK, or
// the status and message the frame call would give; queues nothing, changes nothing.
int check_accum_frame(const MirtContext* ctx, const MirtParams* params);

}  // namespace mirt
