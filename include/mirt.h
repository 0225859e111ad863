/*
 * mirt.h — C ABI of the MI355X-native per-pixel sphere ray tracer.
 *
 * This is the drop-in boundary for ONE hot path of linuxing3/weekend-raytracer-wgpu:
 * the body of `Layer::set_data` (reference src/raytracer/layer.rs:264-282) and everything it
 * calls.  A Rust `Layer` keeps its method surface and replaces the pixel loop with one call
 * into this library (binding shown in INTEGRATION.md).  All structs below are byte-identical
 * to the reference's `#[repr(C)] + bytemuck::Pod` types, so a Rust `&[T]` can be passed as
 * `(ptr, len)` with no marshalling.
 *
 * Conventions
 *   - every entry point returns 0 (MIRT_OK) or a negative MirtStatus; nothing unwinds or
 *     aborts across the ABI; mirt_last_error() returns a thread-local message.
 *   - the caller owns every input pointer for the duration of the call only; the library
 *     never retains caller pointers.  Output buffers are caller-allocated.
 *   - images are row-major, top row first, RGBA8 (A = 255): the format the reference's
 *     consumer `Layer::register_texture` uploads (layer.rs:150-176, `to_rgba8`).
 *   - there is NO CPU fallback behind these symbols: without a HIP device every render call
 *     fails with MIRT_ERR_NO_DEVICE.
 *   - threading: a context is used from one host thread at a time.  Its render calls may be queued
 *     on DIFFERENT HIP streams and overlap on the device: every launch owns its work dispenser and
 *     work counters, and carries the camera it was issued with.  Two exceptions, both about the
 *     context's single accumulation buffer: mirt_ctx_accum_add calls must be ordered with respect to
 *     each other by the caller (same stream, or events), and mirt_ctx_set_scene waits for the device.
 *   - tuning knobs (MIRT_POOL_CONFIG, MIRT_GSS_*, ...) are read from the environment once, in
 *     mirt_ctx_create; render calls never consult the environment.
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_VERSION_MAJOR 0
#define MIRT_VERSION_MINOR 4
#define MIRT_VERSION_PATCH 0

/* ------------------------------------------------------------------------------------------
 * Wire structs (reference file:line of the Rust type each one mirrors)
 * ---------------------------------------------------------------------------------------- */

/* `pub struct Sphere(glm::Vec4, f32, u32, [u32; 2])` — src/raytracer/mod.rs:418-431. 32 B. */
typedef struct MirtSphere {
    float    center[4];     /* xyz + w(=0), `glm::vec3_to_vec4(&center)` mod.rs:429 */
    float    radius;
    uint32_t material_idx;
    uint32_t _pad[2];
} MirtSphere;

/* `pub struct TextureDescriptor { width, height, offset }` — mod.rs:869-876. 12 B.
 * `offset` indexes the flat texel table in units of texels ([f32;3]).
 * The "empty" descriptor is {0, 0, 0xffffffff} (mod.rs:878-886). */
typedef struct MirtTextureDescriptor {
    uint32_t width;
    uint32_t height;
    uint32_t offset;
} MirtTextureDescriptor;

/* `struct GpuMaterial { id, desc1, desc2, x }` — mod.rs:757-765. 32 B.
 * id: 0 lambertian, 1 metal, 2 dielectric, 3 checkerboard (mod.rs:768-813).
 * x:  fuzz (metal) or refraction index (dielectric). */
typedef struct MirtMaterial {
    uint32_t              id;
    MirtTextureDescriptor desc1;
    MirtTextureDescriptor desc2;
    float                 x;
} MirtMaterial;

/* `pub struct GpuCamera` — mod.rs:681-697. 96 B. Produced on the host by
 * `GpuCamera::new` (mod.rs:700-741) == mirt_camera_new() below. */
typedef struct MirtGpuCamera {
    float eye[3];               float _padding1;
    float horizontal[3];        float _padding2;
    float vertical[3];          float _padding3;
    float u[3];                 float _padding4;
    float v[3];                 float lens_radius;
    float lower_left_corner[3]; float _padding5;
} MirtGpuCamera;

/* `struct GpuSkyState` — mod.rs:888-896. 144 B. Opaque Hosek-Wilkie state produced by the
 * hw-skymodel crate on the Rust side (mod.rs:567-595); consumed by raytracer.wgsl:316-343. */
typedef struct MirtSkyState {
    float    params[27];
    float    radiances[3];
    uint32_t _padding[2];
    float    sun_direction[4];
} MirtSkyState;

/* `pub struct Camera { eye_pos, eye_dir, up, vfov: Angle, aperture, focus_distance }` —
 * mod.rs:489-499 (Angle is a newtype over f32 radians, angle.rs:1-4). 48 B. */
typedef struct MirtCamera {
    float eye_pos[3];
    float eye_dir[3];
    float up[3];
    float vfov_radians;
    float aperture;
    float focus_distance;
} MirtCamera;

/* `pub struct SamplingParams` — mod.rs:597-603. 12 B. */
typedef struct MirtSamplingParams {
    uint32_t max_samples_per_pixel;
    uint32_t num_samples_per_pixel;
    uint32_t num_bounces;
} MirtSamplingParams;

/* The state `Layer` holds when `set_data` runs (layer.rs:37-46): camera, world (gathered from
 * `Vec<Box<Sphere>>` into one contiguous slice), material_data, global_texture_data. */
typedef struct MirtScene {
    const MirtGpuCamera* camera;
    const MirtSphere*    spheres;
    uint32_t             n_spheres;
    const MirtMaterial*  materials;
    uint32_t             n_materials;
    const float*         texels;      /* [n_texels][3] f32, `Vec<[f32;3]>` layer.rs:44 */
    uint64_t             n_texels;
    const MirtSkyState*  sky;         /* nullable; required only with MIRT_FLAG_SKY_HOSEK */
} MirtScene;

/* Render modes. */
enum {
    /* `layer.rs` semantics, bit-faithful, every quirk preserved. */
    MIRT_MODE_PARITY = 0,
    /* Full path tracer with the behaviours of raytracer.wgsl:105-521. */
    MIRT_MODE_PT = 1
};

/* Most samples per pixel ONE render / accum_add call takes (MIRT_ERR_SPP_RANGE above): the kernels count the work items of a unit --
 * up to 64 pixels x spp -- in 32 bits.  The reference's UI offers 1..=64 per frame and accumulates to max_samples_per_pixel (mod.rs:599-613). */
#define MIRT_MAX_SPP_PER_CALL (1u << 24)

/* Flags (MIRT_MODE_PT only, except MIRT_FLAG_COUNT_WORK which both modes honour). */
enum {
    MIRT_FLAG_SKY_HOSEK      = 1u << 0, /* sky = Hosek-Wilkie blob (wgsl:154-166,316-343); default: RTIOW gradient */
    MIRT_FLAG_NO_TONEMAP     = 1u << 1, /* skip uncharted2 (wgsl:83-103) */
    MIRT_FLAG_NO_SRGB        = 1u << 2, /* skip the sRGB OETF the Bgra8UnormSrgb surface applies (main.rs:465) */
    MIRT_FLAG_COUNT_WORK     = 1u << 3, /* run the counting build of the kernel: fills MirtStats work counters */
    /* Scheduling of the path-traced kernel (the image is bit-identical either way).  Default: the pooled kernel
     * (paths queued by shading routine in LDS) from a measured number of samples per pixel on -- 32 for scenes with
     * several shading routines, 16 for many-sphere scenes; scenes with ONE routine only on frames below 1 Mpixel, from
     * 800 (csrc/mirt_kernels.h, kPoolMinSpp*) -- and the strip kernel below: lane = pixel (from 16 samples per pixel on
     * in flat scenes its streaming build, render_pt_stream_kernel), lane = sample for counting launches.
     * In parity mode MIRT_FLAG_KERNEL_STRIP forces the lane = sample schedule (default: lane = pixel, the shape of the
     * reference's 2-spp operating point, at every sample count); the image is the same. */
    MIRT_FLAG_KERNEL_STRIP   = 1u << 4, /* force the strip kernel (wave = 64 samples of one pixel) */
    MIRT_FLAG_KERNEL_POOL    = 1u << 5, /* force the pooled kernel */
    MIRT_FLAG_NO_GRID        = 1u << 6, /* many-sphere scenes: scan the flat sphere list instead of the uniform grid */
    /* With MIRT_FLAG_COUNT_WORK on a many-sphere scene: count the work of the grid build that renders such
     * scenes in production (sphere_tests = tests a lane really performs, grid_cells) instead of falling back to
     * the reference's flat scan, whose counters are the oracle's. */
    MIRT_FLAG_COUNT_GRID     = 1u << 7,
    /* OPT-IN fast-math build of the path-traced kernels: hardware v_rcp / v_rsq / v_sqrt / v_sin / v_cos / v_exp /
     * v_log (about 1 ulp) and contraction instead of the bit-exact arithmetic.  Same RNG streams and exact integer
     * accumulation, so the image is deterministic, but pixels may differ from the default build by a few units in
     * the last place: NO parity claim holds with this flag.  Ignored by counting launches and in parity mode. */
    MIRT_FLAG_FAST_MATH      = 1u << 8,
    /* OPT-IN "LDS texel tiles" (BASELINE configs[3]): scenes with an image texture run the pooled kernel's tile build
     * (render_pt_pool_tile_kernel): every wave keeps a 16 x 2 texel window of the texture in LDS, centred on the first
     * image fetch of its strip, and serves the fetches that fall into it from there.  Same texel values, so the image
     * is IDENTICAL to the default build's; measured 3 % slower on config 4, hence opt-in.  A hint: it has
     * no effect where the pooled kernel does not run (few samples per pixel, many-sphere scenes, no image texture).
     * With MIRT_FLAG_COUNT_WORK it fills MirtStats.texel_fetches / texel_tile_hits. */
    MIRT_FLAG_TEXEL_TILES    = 1u << 9
};

/* What one render call computes.  The image is `width x height`; this call renders the rows
 * selected by (row_begin,row_end) and the tile interleave, into a COMPACT buffer of
 * mirt_params_out_rows() rows.  With tile_rows == 0 (or n_parts <= 1) the rows are the
 * contiguous band [row_begin,row_end).  With n_parts > 1 the band is cut into tiles of
 * `tile_rows` rows and this call renders tiles t with t % n_parts == part, in order — the
 * partition used to balance the 8 GPUs of a node. */
typedef struct MirtParams {
    uint32_t width;        /* `vp_size[0] as u32` layer.rs:270-275 */
    uint32_t height;
    uint32_t spp;          /* `sampling.num_samples_per_pixel` layer.rs:316; 1 .. MIRT_MAX_SPP_PER_CALL (progressive accumulation adds calls up) */
    uint32_t num_bounces;  /* PT mode; SamplingParams.num_bounces mod.rs:602 */
    uint32_t mode;         /* MIRT_MODE_* */
    uint32_t flags;        /* MIRT_FLAG_* */
    uint64_t seed;         /* PT mode RNG seed; 0 reproduces the WGSL stream (wgsl:498-502) */
    uint32_t row_begin;    /* band; row_end == 0 means `height` */
    uint32_t row_end;
    uint32_t tile_rows;    /* 0 = no interleave */
    uint32_t n_parts;
    uint32_t part;
    uint32_t sample_begin; /* PT: first sample index (progressive accumulation); normally 0 */
    /* PT: 0 (default) = every sample has its own RNG stream, that of frame_number = sample + 1 at one sample per
     * frame -- the image then does not depend on how samples are grouped into launches.  n > 0 = the REFERENCE's
     * stream for `num_samples_per_pixel` = n: frame f = sample / n + 1 seeds the pixel's RNG once (initRng,
     * wgsl:498-502) and its n samples draw from that one stream in turn (samplePixel, wgsl:105-122), exactly as
     * Raytracer::render_frame advances (mod.rs:303-351, 626-670).  Needs spp % n == 0 and sample_begin % n == 0;
     * runs on the lane-per-pixel schedule (a pixel's samples are then sequentially dependent).  Frame numbers count from
     * sample 0 of the accumulation plus `frame_begin` (below): the reference's frame_number survives
     * render_progress.reset() (mod.rs:284, 385), so accumulations after the first start at a later frame. */
    uint32_t frame_spp;
    /* PT with frame_spp > 0: the frames the reference's Raytracer had rendered BEFORE sample 0 of this accumulation, i.e. its
     * `frame_number - 1` at the reset -- `frame_number` starts at 1, advances with every render_frame call (completed frames
     * included) and survives `render_progress.reset()` (mod.rs:284, 350, 385).  Sample s then draws from the stream of frame
     * frame_begin + s / frame_spp + 1.  0 = a freshly constructed Raytracer.  Ignored when frame_spp == 0. */
    uint32_t frame_begin;
} MirtParams;

/* Work counters of the last render on a context (rocprof-independent).  The ray/test/scatter
 * counters are filled only when MIRT_FLAG_COUNT_WORK was set.  Parity mode counts what the reference's
 * sequential sample loop executes (it returns at the first terminating sample, layer.rs:333-374):
 * lane_iterations = samples executed, scatter[1] = scatter_metal calls. */
typedef struct MirtStats {
    double   kernel_ms;        /* hipEvent time of the render kernel of the LAST render call */
    double   kernel_ms_total;  /* summed over every render call since the previous mirt_ctx_get_stats */
    uint64_t launches;         /* number of render calls in kernel_ms_total */
    uint64_t samples;          /* pixels x spp rendered by the last call */
    uint64_t rays;             /* rays traced (primary + scattered) */
    uint64_t sphere_tests;     /* ray-sphere discriminant evaluations */
    uint64_t roots;            /* quadratic roots evaluated */
    uint64_t hits;             /* hit records built */
    uint64_t scatter[5];       /* lambertian, metal, dielectric, checkerboard, missing-material */
    uint64_t sky_misses;       /* rays that left the scene */
    uint64_t lane_iterations;  /* PT: active lanes summed over bounce-loop iterations */
    uint64_t wave_iterations;  /* PT: bounce-loop iterations summed over waves (x64 = lane slots) */
    uint64_t grid_cells;       /* MIRT_FLAG_COUNT_GRID: grid cells visited, summed over lanes (MIRT_SCENE_HBM: BVH nodes visited, leaves included) */
    uint64_t grid_wave_cells;  /* MIRT_FLAG_COUNT_GRID: cell-loop iterations summed over waves (x64 = lane slots; MIRT_SCENE_HBM: BVH loop iterations) */
    uint64_t texel_fetches[2];   /* MIRT_FLAG_TEXEL_TILES: image-texel fetches at [0] camera-ray hits, [1] later bounces */
    uint64_t texel_tile_hits[2]; /* ... of those, served by the wave's LDS tile */
} MirtStats;

typedef enum MirtStatus {
    MIRT_OK                      =  0,
    /* mirrors RenderParamsValidationError, mod.rs:396-411 / RenderParams::validate mod.rs:450-484 */
    MIRT_ERR_MAX_SAMPLES_MULTIPLE = -1, /* MaxSampleCountNotMultiple */
    MIRT_ERR_VIEWPORT_SIZE        = -2, /* ViewportSize */
    MIRT_ERR_VFOV_RANGE           = -3, /* VfovOutOfRange */
    MIRT_ERR_APERTURE_RANGE       = -4, /* ApertureOutOfRange */
    MIRT_ERR_FOCUS_DISTANCE       = -5, /* FocusDistanceOutOfRange */
    MIRT_ERR_SKY                  = -6, /* HwSkyModelValidationError / sky blob missing */
    /* library-level */
    MIRT_ERR_NULL_POINTER         = -10,
    MIRT_ERR_SPP_ZERO             = -11,
    MIRT_ERR_BAD_MODE             = -12,
    MIRT_ERR_BAD_ROWS             = -13,
    MIRT_ERR_MATERIAL_INDEX       = -14, /* sphere.material_idx >= n_materials, or parity mode with n_materials < 3 (layer.rs:345-349 reads material_data[2]) */
    MIRT_ERR_TEXEL_RANGE          = -15, /* a descriptor reaches past n_texels */
    MIRT_ERR_OUT_BUFFER           = -16, /* out_len too small */
    MIRT_ERR_NO_SCENE             = -17,
    /* The kernels keep the scene in LDS (160 KB per CU, 120 KB = 122 880 B of it for the scene): a scene is accepted if one
     * of two layouts fits, else mirt_ctx_set_scene fails with this code.  (The reference's own buffers are bounded by wgpu's
     * 512 MiB storage-buffer limit, main.rs:421-481; BASELINE's largest scene has 484 spheres.)
     *   flat layout (every mode and flag): 96 + 32 * n_spheres + 48 * n_materials + 144 <= 122 880 bytes
     *       -- e.g. 3 831 spheres with one material;
     *   grid layout (MIRT_MODE_PT only, scenes of >= 32 spheres of which at most 64 exceed 4 median radii): n_spheres <= 4 095
     *       (12-bit sphere ids in a path's state word), <= 4 096 cells and <= 65 535 cell entries (the host starts at a cell of
     *       2.5 median radii and coarsens it, x 1.26 per step up to 4, while either limit is exceeded or the blob would cost the
     *       pooled kernel its 152-slot geometry), and 240 + blob <= 122 880 bytes with blob ~ 17 * n_spheres + 8 * cells +
     *       2 * (entries beyond the first two of each cell).  A blob that leaves the pooled kernel no
     *       room for its path pools (mirt_grid_plan: pool_slots = 0) runs the strip kernel's grid build.  mirt_grid_plan() answers "which grid would this scene get" without a device.
     * A scene that fits ONLY the grid layout renders in path-traced mode with default flags; a render call in parity mode, or
     * with MIRT_FLAG_COUNT_WORK without MIRT_FLAG_COUNT_GRID, or with MIRT_FLAG_NO_GRID, returns this code.
     * A world that fits neither layout is set with MIRT_SCENE_HBM (mirt_ctx_set_scene_ex below): its tables stay in device memory
     * and a BVH replaces the grid, up to MIRT_SCENE_HBM_MAX_SPHERES spheres; above that, set_scene_ex returns this code too. */
    MIRT_ERR_SCENE_TOO_LARGE      = -18,
    MIRT_ERR_FRAME_SPP            = -19, /* frame_spp does not divide spp / sample_begin */
    MIRT_ERR_NO_DEVICE            = -20,
    MIRT_ERR_HIP                  = -21,
    MIRT_ERR_ALLOC                = -22,
    MIRT_ERR_SPP_RANGE            = -24, /* spp > MIRT_MAX_SPP_PER_CALL, or sample_begin (the samples accumulated so far) + spp reaches 2^32 */
    MIRT_ERR_IMAGE_DECODE         = -23  /* mirt_jpeg_*: not a JPEG this decoder handles (TextureError::ImageLoadError, texture.rs:193-199) */
} MirtStatus;

typedef struct MirtContext MirtContext; /* opaque: one per device; owns all device memory */

/* ------------------------------------------------------------------------------------------
 * Entry points
 * ---------------------------------------------------------------------------------------- */

/* Packed version (major<<16 | minor<<8 | patch). */
uint32_t    mirt_version(void);
/* Thread-local description of the last failure on this thread ("" if none). */
const char* mirt_last_error(void);
/* Static name of a status code. */
const char* mirt_status_string(int status);

/* `RenderParams::validate` (mod.rs:450-484) over the fields that reach this path. */
int mirt_validate_render_params(const MirtCamera* camera, const MirtSamplingParams* sampling,
                                uint32_t viewport_w, uint32_t viewport_h);

/* `GpuCamera::new(&camera, viewport_size)` (mod.rs:700-741).  Host-side set-up arithmetic in
 * f32 exactly as the reference does it; runs once per image, not part of the hot loop. */
int mirt_camera_new(const MirtCamera* camera, uint32_t viewport_w, uint32_t viewport_h,
                    MirtGpuCamera* out);

/* `camera_orientation` + `FlyCameraController::renderer_camera` (fly_camera.rs:52-64,227-241):
 * pose (position, yaw, pitch in radians) -> Camera. */
int mirt_camera_from_fly_pose(const float position[3], float yaw_radians, float pitch_radians,
                              float vfov_degrees, float aperture, float focus_distance,
                              MirtCamera* out);

/* `Angle::degrees(d).as_radians()` (angle.rs:8-12): d * PI / 180 in f32. */
float mirt_degrees_to_radians(float degrees);
/* `Angle::as_degrees` (angle.rs:20-22): r * 180 / PI in f32. */
float mirt_radians_to_degrees(float radians);

/* Number of rows a render call with these params writes (0 on invalid params). */
uint32_t mirt_params_out_rows(const MirtParams* params);
/* Absolute image row of compact output row `i` (UINT32_MAX if out of range). */
uint32_t mirt_params_out_row_index(const MirtParams* params, uint32_t i);

/* The uniform grid mirt_ctx_set_scene would build over these spheres (many-sphere scenes, path-traced mode): HOST-ONLY -- no
 * device, no context.  `lds_bytes_per_block` = LDS a workgroup may use (0 = gfx950's 163 840).  cell_factor = the cell edge in
 * median radii the coarsening rule settles on (0 = no grid: fewer than 32 spheres, nothing small enough to bin, more than 64
 * big spheres, or more than 65 535 cell entries even at the coarsest cell); pool_slots = path slots per wave the pooled kernel's
 * grid build would run beside that blob (0 = it does not fit: strip kernel). */
typedef struct MirtGridPlan {
    float    cell_factor;
    uint32_t blob_bytes;
    uint32_t n_cells;
    uint32_t n_entries;
    uint32_t n_big;
    uint32_t pool_slots;
} MirtGridPlan;
int mirt_grid_plan(const MirtSphere* spheres, uint32_t n_spheres, uint64_t lds_bytes_per_block, MirtGridPlan* out);

/* Create / destroy a context on HIP device `device` (ordinal as seen by this process). */
int  mirt_ctx_create(int device, MirtContext** out);
void mirt_ctx_destroy(MirtContext* ctx);

/* Validate and upload the scene into device memory owned by the context (what
 * `Layer::new` + `set_global_data` leave in `self`, layer.rs:49-148).  The scene stays
 * resident across render calls until replaced. */
int mirt_ctx_set_scene(MirtContext* ctx, const MirtScene* scene);
/* ---- worlds beyond the LDS budget: the scene's tables in device memory, nearest hit through a BVH ----
 * flags == 0: exactly mirt_ctx_set_scene.  MIRT_SCENE_HBM keeps the spheres, materials and a BVH over the spheres in device memory
 * whatever the scene's size (small scenes too, so that the path can be compared with the LDS builds); LDS then holds the camera,
 * the sky and the traversal stacks.  At most MIRT_SCENE_HBM_MAX_SPHERES spheres (512 MiB of 32-byte spheres, the reference's
 * storage-buffer size, main.rs:448), checked before any sphere is read: MIRT_ERR_SCENE_TOO_LARGE.  Unknown flag bits:
 * MIRT_ERR_BAD_MODE; a failed allocation: MIRT_ERR_ALLOC.  Failure-atomic like mirt_ctx_set_scene (a refused call leaves the previous
 * scene in place; a failure after validation leaves no scene).
 * Render calls on such a scene keep every meaning of MirtParams; the image is byte-identical to the flat scan's:
 *   default                     lane-per-pixel strip kernel with BVH traversal (render_pt_hbm_kernel<COUNT,HOSEK,true,BY_PIXEL>);
 *   MIRT_FLAG_FAST_MATH         the fast-math compilation of the same kernel ("fast_build::" + its name);
 *   MIRT_FLAG_NO_GRID           the flat scan of the sphere table in device memory (render_pt_hbm_kernel<...,false,...>);
 *   MIRT_FLAG_COUNT_WORK        alone: counts that flat scan (every counter equals the oracle's); with MIRT_FLAG_COUNT_GRID: counts the
 *                               BVH build (sphere_tests = tests performed, grid_cells / grid_wave_cells = BVH nodes visited);
 *   MIRT_FLAG_KERNEL_POOL       on the BVH build (no MIRT_FLAG_NO_GRID; counting launches: with MIRT_FLAG_COUNT_GRID): the pooled schedule,
 *                               render_pt_pool_hbm_kernel<THREADS,SLOTS,MINW,COUNT,HOSEK> (a progressive frame: render_pt_pool_hbm_frame_kernel;
 *                               MIRT_FLAG_FAST_MATH: "fast_build::" + the name) -- a wave keeps a pool of paths in LDS and refills the lanes
 *                               whose paths have ended instead of idling them.  Same image, same sums.  OPT-IN: no sample
 *                               count selects it by default.  Not pooled, and run exactly as without the flag: num_bounces > 255,
 *                               frame_spp > 0, and a tree so deep that no geometry fits LDS (mirt_bvh_pool_plan: slots == 0);
 *   MIRT_FLAG_KERNEL_STRIP      wins over _POOL as everywhere else: the default kernel;  MIRT_FLAG_TEXEL_TILES: ignored;
 *   parity mode                 the layer.rs flat scan with the spheres in device memory (render_parity_hbm_kernel).
 * The BVH: binned SAH over the sphere centres, binary, leaves of at most MIRT_BVH_MAX_LEAF spheres, depth at most MIRT_BVH_MAX_DEPTH by
 * construction; up to MIRT_BVH_MAX_ALWAYS spheres (those larger than MIRT_BVH_BIG_RADII median radii, and those whose box is not finite)
 * are tested for every ray instead.  Deterministic, built on at most 16 host threads.
 * MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE builds the tree on the device instead (the flag alone: MIRT_ERR_BAD_MODE): the same
 * always-tested list (host, O(n)), the other spheres sorted by the Morton code of their centre and split top-down, level by level, where
 * the code's highest differing bit flips -- at the object median where the codes are equal or the split would break the depth limit.
 * Same node layout, leaf size and depth limit, the host formula's boxes, so the image is byte-identical to the host tree's; the
 * tree is a different one and culls somewhat less.  Deterministic; synchronous like every set_scene. */
enum {
    MIRT_SCENE_HBM        = 1u << 0,              /* mirt_ctx_set_scene_ex / mirt_node_set_scene_ex flags */
    MIRT_SCENE_BVH_DEVICE = 1u << 1               /* only together with MIRT_SCENE_HBM: build the BVH on the device */
};
#define MIRT_SCENE_HBM_MAX_SPHERES (1u << 24)
#define MIRT_BVH_MAX_DEPTH  32                    /* levels below the root; sizes the kernels' traversal stacks */
#define MIRT_BVH_MAX_LEAF   4
#define MIRT_BVH_MAX_ALWAYS 64
#define MIRT_BVH_BIG_RADII  4
int mirt_ctx_set_scene_ex(MirtContext* ctx, const MirtScene* scene, uint32_t flags);
/* What the BVH of those spheres would be: HOST-ONLY (no device, no context), the same tree set_scene_ex builds.
 *   n_nodes          inner nodes (== n_leaves - 1 for a non-empty tree), 64 bytes each (both child boxes in the parent)
 *   n_leaves         leaves; n_leaf_spheres spheres in them, n_always on the always-tested list (n_leaf_spheres + n_always == n_spheres)
 *   max_depth        deepest leaf (root = 0), <= MIRT_BVH_MAX_DEPTH;  max_leaf = largest leaf, <= MIRT_BVH_MAX_LEAF
 *   device_bytes     64 * n_nodes + 20 * n_spheres: nodes, test records {centre, r^2} and original sphere ids (u32), always list first
 * MIRT_ERR_SCENE_TOO_LARGE above MIRT_SCENE_HBM_MAX_SPHERES. */
typedef struct MirtBvhPlan {
    uint32_t n_nodes, n_leaves, n_leaf_spheres, n_always, max_depth, max_leaf;
    uint64_t device_bytes;
} MirtBvhPlan;
int mirt_bvh_plan(const MirtSphere* spheres, uint32_t n_spheres, MirtBvhPlan* out);
/* The tree a context holds (either builder): its counts as mirt_bvh_plan reports them (for a host-built tree: equal to mirt_bvh_plan of
 * the same spheres), the root reference, and the traversal bounds.  MIRT_ERR_NO_SCENE without a MIRT_SCENE_HBM scene. */
typedef struct MirtBvhInfo {
    MirtBvhPlan plan;            /* of the tree in the context (either builder) */
    uint32_t    root;
    uint32_t    built_on_device;
    float       centre[3], radius, r_max;
} MirtBvhInfo;
int mirt_ctx_bvh_info(MirtContext* ctx, MirtBvhInfo* out);
/* The geometry MIRT_FLAG_KERNEL_POOL would run on a MIRT_SCENE_HBM scene whose tree is `max_depth` deep (MirtBvhInfo.plan.max_depth):
 * HOST-ONLY, the function the launch itself uses.  hosek != 0: the launch stages the Hosek sky.  lds_bytes_per_cu = LDS of a compute
 * unit (0 = gfx950's 163 840).  A block holds the camera (96 bytes, + 144 of sky) and, per wave of 64 threads, a pool of
 * 50 * slots + 384 bytes and 64 traversal stacks of stack_entries == max_depth node references (256 * max_depth bytes):
 *   lds_bytes_per_block = 96 (+ 144) + threads / 64 * (50 * slots + 384 + 256 * max_depth),
 *   waves_per_cu        = waves the launch keeps resident per compute unit: whole blocks, at most 16 waves.
 * The rule: of the slot counts 112, 96, 80 and 64 the largest that leaves 16 waves resident; where none does, the one that keeps most
 * waves (the larger pools on a tie).  slots == 0 (all fields 0): not one block fits, and the launch runs the strip kernel.
 * MIRT_ERR_NULL_POINTER: out is null;  MIRT_ERR_BAD_ROWS: max_depth > MIRT_BVH_MAX_DEPTH. */
typedef struct MirtBvhPoolPlan { uint32_t threads, slots, waves_per_cu, stack_entries, lds_bytes_per_block; } MirtBvhPoolPlan;
int mirt_bvh_pool_plan(uint32_t max_depth, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtBvhPoolPlan* out);
/* Copies the tree to the host: plan.n_nodes nodes of 64 bytes {left box min[3] max[3], right box min[3] max[3], left, right, 2 x u32 pad}
 * (a reference with bit 31 set is a leaf: bits 24..30 = sphere count, bits 0..23 = first record), 4 floats {centre, r * r} per sphere and
 * the original index of every record (always-tested list first).  Blocking; meant for tests, like mirt_ctx_accum_read.
 * MIRT_ERR_OUT_BUFFER if a buffer is too small (nodes_bytes in bytes, recs_len in floats, ids_len in entries). */
int mirt_ctx_bvh_read(MirtContext* ctx, void* nodes, size_t nodes_bytes, float* recs, size_t recs_len, uint32_t* ids, size_t ids_len);
/* ---- moving the spheres of a MIRT_SCENE_HBM scene in place ----
 * Spheres first .. first + count of the context's MIRT_SCENE_HBM scene take center[0..3] and radius from the `count` records given
 * (MirtSphere, 32 bytes each).  material_idx and the padding of the input are NOT READ: a sphere keeps its material, so everything a
 * scene's materials decide stays valid.  r * r and 1 / r are computed on the device with the single IEEE operations set_scene uses.
 * The tree keeps its topology and its always-tested list (a performance rule: a tree sphere that grows, or becomes non-finite, stays in
 * the tree); every child box is recomputed bottom-up by the host formula and the traversal bounds are reduced again, always over the
 * whole tree, whichever builder made it.  The image is byte-identical to the flat scan's and to a fresh set_scene_ex of the moved
 * world; a tree whose spheres moved far culls worse (mirt_ctx_bvh_refits tells a host how often it has refitted; rebuild with
 * set_scene_ex).
 * Like set_scene the call first waits for the device -- renders in flight on caller streams, and whatever was queued to produce
 * d_spheres -- and returns when the tree is ready.  The accumulation buffer is not touched (reset it, as after set_camera).
 *   mirt_ctx_update_spheres          reads `spheres` from host memory;
 *   mirt_ctx_update_spheres_device   reads `d_spheres` from memory of the context's device (4-byte aligned), device to device.
 * MIRT_ERR_NULL_POINTER: ctx is null, or the records are with count > 0;  MIRT_ERR_NO_SCENE: no scene, or not a MIRT_SCENE_HBM one;
 * MIRT_ERR_BAD_ROWS: first + count > n_spheres (in 64 bits);  count == 0: MIRT_OK without device work.  An argument error changes
 * nothing; a failure after the first write leaves the context with no scene. */
int      mirt_ctx_update_spheres(MirtContext* ctx, uint32_t first, uint32_t count, const MirtSphere* spheres);
int      mirt_ctx_update_spheres_device(MirtContext* ctx, uint32_t first, uint32_t count, const void* d_spheres);
/* Successful updates (count > 0) since the scene was set; 0 after every set_scene* and set_spheres*, and for a null ctx. */
uint32_t mirt_ctx_bvh_refits(const MirtContext* ctx);
/* ---- replacing the spheres of a MIRT_SCENE_HBM scene ----
 * The context's MIRT_SCENE_HBM scene gets a new sphere table of `n_spheres` records (MirtSphere, 32 bytes each): center[0..3], radius and
 * -- unlike update_spheres -- material_idx are read; center[3] and _pad are NOT READ.  The count may differ from the resident one and
 * may be 0 (then the pointer may be null).  Camera, materials, texels and sky stay resident and are not uploaded again.  Everything
 * set_scene derives from the spheres is derived again ON THE DEVICE: the material-index check, the census of scatter routines, the
 * always-tested list (the rule above, entry for entry), the prepared spheres, and the tree by the MIRT_SCENE_BVH_DEVICE builder -- whichever
 * builder made the tree before.  Afterwards the context cannot be told from one that received a fresh
 * mirt_ctx_set_scene_ex(MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE) of a scene with these spheres and what it already holds: the bytes of
 * mirt_ctx_bvh_read, mirt_ctx_bvh_info (built_on_device = 1), images, sums, work counters, mirt_ctx_last_kernel, the status of render
 * calls, mirt_ctx_bvh_refits == 0.
 * Like set_scene the call first waits for the device -- renders in flight on caller streams, and whatever was queued to produce
 * d_spheres -- and returns when the tree is ready.  The accumulation buffer is not touched (reset it, as after set_camera).
 *   mirt_ctx_set_spheres          reads `spheres` from host memory (one copy to the device, then the same path);
 *   mirt_ctx_set_spheres_device   reads `d_spheres` from memory of the context's device (4-byte aligned): nothing leaves the device but
 *                                 the census word and the list (under 300 bytes).
 * MIRT_ERR_NULL_POINTER: ctx is null, or the records are with n_spheres > 0;  MIRT_ERR_NO_SCENE: no scene, or not a MIRT_SCENE_HBM one;
 * MIRT_ERR_SCENE_TOO_LARGE: above MIRT_SCENE_HBM_MAX_SPHERES, before any sphere is read.  An argument error changes nothing; a failure
 * after the first write leaves the context with no scene.  A material_idx >= n_materials does not refuse the call: as after set_scene
 * the path-traced render calls answer MIRT_ERR_MATERIAL_INDEX until a set_spheres* or set_scene* without one; the materials' own
 * verdict (MIRT_ERR_TEXEL_RANGE) stays as set_scene found it. */
int      mirt_ctx_set_spheres(MirtContext* ctx, const MirtSphere* spheres, uint32_t n_spheres);
int      mirt_ctx_set_spheres_device(MirtContext* ctx, const void* d_spheres, uint32_t n_spheres);

/* ---- ray queries against a MIRT_SCENE_HBM scene: picking, line of sight, batches of rays ----
 * Every ray gets the answer of the flat scan over the resident sphere table, by the renderer's own arithmetic (the sphere test of the
 * path-traced kernels): `closest` starts at the ray's t_max (pass 1000.0f for exactly what a path of the renderer gets), a sphere wins
 * with f < closest, f = the first computed root above MIN_T = 0.001, and on equal f the lower ORIGINAL index wins.  `direction` is not
 * normalised; t is in units of it.  On a hit: sphere = the original index, t = f, point = fma(t, direction, origin) per component,
 * normal = inv_r * (point - centre) with inv_r the table's single IEEE 1 / r -- what the renderer shades with: NOT turned towards the
 * ray, so it points inwards for a negative radius.  On a miss: sphere = MIRT_RAY_MISS and every other field 0.  Every float bit pattern
 * is legal in a ray (NaN or infinite t_max, a zero direction, non-finite origins): the result is whatever that arithmetic gives, a miss
 * for a NaN t_max or a zero direction, and the tree walk agrees with it bit for bit.  `_pad` is not read.  Materials are never read: a
 * material_idx out of range in the scene does not matter here.
 * flags:
 *   0                   the BVH walk of the render kernels (trace_rays_kernel<true,...>), lane = ray, rays in the caller's order;
 *   MIRT_RAYS_FLAT      the flat scan itself (trace_rays_kernel<false,...>): the comparison build, as MIRT_FLAG_NO_GRID is for renders;
 *   MIRT_RAYS_ANY_HIT   occlusion query: a ray stops at the first sphere it finds with f < t_max and writes sphere = 0 ("something is
 *                       hit") or MIRT_RAY_MISS, every other field 0; hit or miss is exactly that of the nearest-hit query.  Valid with _FLAT;
 *   MIRT_RAYS_COUNT     the counting build: fills the counters of MirtRayStats (otherwise 0).  Same results.
 *   MIRT_RAYS_SORT      the batch is traced in an order the library derives on the device (trace_rays_sorted_kernel<...>; "sorted ray
 *                       batches" below).  Same bytes in the same places.  Valid with every other flag.  Bit 3 is not assigned.
 *   any other bit: MIRT_ERR_BAD_MODE.
 * MIRT_ERR_NULL_POINTER: ctx is null, or rays / hits is with n_rays > 0;  MIRT_ERR_NO_SCENE: no scene, or not a MIRT_SCENE_HBM one (the LDS
 * layouts keep no record table and no tree to query);  n_rays == 0: MIRT_OK without device work.
 *   mirt_ctx_trace_rays          rays and hits in HOST memory: copy, kernel, copy on the context's stream; blocking.
 *   mirt_ctx_trace_rays_device   rays and hits in memory of the context's device (4-byte aligned), queued on `hip_stream` (NULL = the
 *                                context's stream; hipStreamLegacy for the default stream, as for mirt_ctx_render_device), no host
 *                                synchronisation.  The kernel reads the tree as it is when it RUNS; mirt_ctx_set_scene*, _update_spheres*
 *                                and _set_spheres* wait for the device before they write, so they stay ordered after traces in flight.
 * Neither touches the accumulation buffer or MirtStats; mirt_ctx_last_kernel reports the trace kernel afterwards; mirt_ctx_synchronize
 * waits for traces too.  Counting traces (MIRT_RAYS_COUNT) share one counter block: the caller keeps them in order among themselves. */
typedef struct MirtRay    { float origin[3]; float t_max; float direction[3]; float _pad; } MirtRay;      /* 32 B */
typedef struct MirtRayHit { float t; uint32_t sphere; float point[3]; float normal[3]; }   MirtRayHit;    /* 32 B */
#define MIRT_RAY_MISS 0xffffffffu
enum { MIRT_RAYS_FLAT = 1u << 0, MIRT_RAYS_ANY_HIT = 1u << 1, MIRT_RAYS_COUNT = 1u << 2, MIRT_RAYS_SORT = 1u << 4 };     /* bit 3: unassigned */
/* Of the LAST trace call.  kernel_ms: hipEvent time of its kernel, 0 with mirt_ctx_set_timing(ctx, 0).  The counters are filled by
 * MIRT_RAYS_COUNT only: rays traced, sphere tests the lanes really performed, roots evaluated, rays with a hit, BVH nodes visited summed
 * over lanes (leaves included) and BVH loop iterations summed over waves (x 64 = lane slots) -- both 0 for the flat scan. */
typedef struct MirtRayStats { double kernel_ms; uint64_t rays, sphere_tests, roots, hits, nodes, wave_nodes; } MirtRayStats;
int mirt_ctx_trace_rays(MirtContext* ctx, const MirtRay* rays, uint32_t n_rays, uint32_t flags, MirtRayHit* hits);
int mirt_ctx_trace_rays_device(MirtContext* ctx, const void* d_rays, uint32_t n_rays, uint32_t flags, void* d_hits, void* hip_stream);
/* Waits for the last trace call and reports its statistics (all 0 before the first). */
int mirt_ctx_trace_stats(MirtContext* ctx, MirtRayStats* out);

/* ---- first-hit feature frames of a MIRT_SCENE_HBM scene: albedo, normal, depth and id per pixel ----
 * What the context's camera sees FIRST at every pixel, for denoiser guides (albedo, normal) and for picking, outlines and snapping
 * (sphere, t).  One MirtFeaturePixel per pixel of the rows `params` selects, compact and row-major exactly like mirt_ctx_render
 * (row_begin / row_end / tile_rows / n_parts / part; mirt_params_out_rows gives the row count).  Of MirtParams the call reads width,
 * height, the row fields, spp, sample_begin and seed; it does NOT read mode, num_bounces, flags and frame_begin.  frame_spp must be 0
 * (MIRT_ERR_FRAME_SPP otherwise): the reference's per-frame stream threads a pixel's later primary rays through the bounces of its
 * earlier paths, and a feature pass has no paths -- a guide needs the same pixel filter, not the same draws.
 *   the centre ray   u = (x + 0.5f) * inv_w, v = 1 - (y + 0.5f) * inv_h with inv_w = 1.0f / (float)width, inv_h = 1.0f / (float)height;
 *                    origin = eye (the lens is ignored, no random draw), direction = fma(v, vertical, fma(u, horizontal,
 *                    lower_left_corner)) - eye per component: the renderer's primary ray with both jitter draws replaced by 0.5 and a
 *                    zero lens.  mirt_camera_pixel_ray restates it on the host bit for bit.
 *   sphere, t        the nearest hit of the centre ray from t_max = 1000, the `sphere` and `t` of mirt_ctx_trace_rays: the original
 *                    index and the computed root, or MIRT_RAY_MISS and 0.
 *   the sample set   spp == 0 (legal here): the centre ray alone.  spp >= 1: the renderer's own primary rays of samples
 *                    sample_begin .. sample_begin + spp - 1, the RNG seeded from `seed` as a render call seeds it -- jitter, lens,
 *                    the two lens draws: the guides carry the pixel filter and the depth of field of the beauty pass.  A pixel costs
 *                    1 ray at spp == 0 and spp + 1 rays otherwise.
 *   albedo, normal   float sums from +0 over the samples in order; a sample that hits adds its normal inv_r * (point - centre) (NOT
 *                    turned towards the ray, as in MirtRayHit) and its albedo, a sample that misses adds nothing; the record holds
 *                    sum / (float)max(spp, 1).  A NaN stays a NaN (a zero-radius winner: inf x 0).  The albedo of a hit is the
 *                    attenuation the renderer's scatter routine of its material applies, without the lambertian's grazing factor:
 *                    routines 0 and 1 the first texture at the hit, 2 (1, 1, 1), 3 the checkerboard's texture of the hit point,
 *                    any other id (0.9921, 0.24705, 0.57254).  No scatter direction is computed and no further draw is taken.
 * flags: 0 = the BVH walk of the render kernels (feature_frame_kernel<true>); MIRT_FEATURES_FLAT = the flat scan of the resident table
 * in original index order, the comparison build as MIRT_RAYS_FLAT is; any other bit: MIRT_ERR_BAD_MODE.
 * MIRT_ERR_NULL_POINTER: ctx, params or the output is null;  MIRT_ERR_NO_SCENE: no scene, or not a MIRT_SCENE_HBM one;  zero width or
 * height and bad rows: the codes mirt_ctx_render gives;  MIRT_ERR_SPP_RANGE: spp > MIRT_MAX_SPP_PER_CALL or sample_begin + spp reaches
 * 2^32;  MIRT_ERR_OUT_BUFFER: out_len < rows * width * 32;  MIRT_ERR_MATERIAL_INDEX / MIRT_ERR_TEXEL_RANGE: exactly as a path-traced
 * render call on that scene answers -- this call reads materials, unlike ray queries.  A refused call queues nothing; neither does a
 * call whose part of a tile partition owns no row (MIRT_OK).
 *   mirt_ctx_render_features          `out` in HOST memory: kernel and copy on the context's stream; blocking.
 *   mirt_ctx_render_features_device   `d_out` in memory of the context's device (4-byte aligned): ONE kernel queued on `hip_stream` (NULL =
 *                                     the context's stream; hipStreamLegacy for the default stream), no host synchronisation.
 * State is kept the way the ray queries keep it: neither the launch ring, MirtStats nor the accumulation is touched; mirt_ctx_last_kernel
 * names the feature kernel; mirt_ctx_synchronize and mirt_ctx_destroy wait for it; its time is mirt_ctx_trace_stats().kernel_ms (the
 * counters are 0).
 *   mirt_camera_pixel_ray             HOST ONLY, no device: the centre ray of pixel (x, y) of a width x height viewport (row 0 on top) in
 *                                     float32 with fmaf, t_max = 1000.0f.  MIRT_ERR_NULL_POINTER for a null pointer,
 *                                     MIRT_ERR_VIEWPORT_SIZE for a zero size, MIRT_ERR_BAD_ROWS for a pixel outside the viewport. */
typedef struct MirtFeaturePixel { float albedo[3]; float t; float normal[3]; uint32_t sphere; } MirtFeaturePixel;   /* 32 B */
enum { MIRT_FEATURES_FLAT = 1u << 0 };
int mirt_ctx_render_features(MirtContext* ctx, const MirtParams* params, uint32_t flags, MirtFeaturePixel* out, size_t out_len);
int mirt_ctx_render_features_device(MirtContext* ctx, const MirtParams* params, uint32_t flags, void* d_out, size_t out_len, void* hip_stream);
int mirt_camera_pixel_ray(const MirtGpuCamera* camera, uint32_t width, uint32_t height, uint32_t x, uint32_t y, MirtRay* out);

/* ---- path-traced radiance for a caller's rays against a MIRT_SCENE_HBM scene ----
 * The path tracer for rays the HOST chooses: panorama, fisheye, cube-map and stereo cameras, light and reflection probes, irradiance
 * at points of a simulation, batches of training rays held in device memory.  One MirtRadiance per MirtRadianceRay, in the caller's order.
 *   a sample         is the renderer's sample from its primary ray on.  For sample s in sample_begin .. sample_begin + spp - 1 the ray's
 *                    lane seeds rng.state = jenkins_hash((ray.stream ^ jenkins_hash(s + 1)) ^ seed_mix), seed_mix derived from `seed`
 *                    exactly as a render call derives it: `stream` takes the place the pixel index (x + y * width) has in a render.  The
 *                    lane then advances the stream by the four draws a primary ray consumes (two jitter, two lens) and runs the renderer's
 *                    bounce loop from (origin, direction) with num_bounces.  So a ray equal to a renderer's primary ray, with `stream`
 *                    equal to that pixel's index, continues that sample's path bit for bit.
 *   the ray          `direction` is used as given, NOT normalised, as a primary ray's is; every segment of the path has the renderer's
 *                    t_max = 1000; `_pad` is not read.
 *   the record       sum[k] = the sum over the samples, in order, of to_fixed(radiance[k]): the units of the context's accumulation
 *                    buffer, 2^-20, each sample clamped to [0, 4096).  Without MIRT_RADIANCE_ACCUMULATE the record is overwritten:
 *                    samples = spp, _pad = 0.  With it the lane adds to the sums already in the record and adds spp to `samples`
 *                    (mod 2^32; _pad = 0); a progressive probe passes sample_begin = the samples so far, as mirt_ctx_accum_add does
 *                    internally.  The mean is sum / 2^20 / samples; it is left to the host, because the integer sums are what is exact
 *                    and additive.  A record depends only on its ray, the params and the scene: not on the ray's place in the batch, not
 *                    on n_rays.
 * flags: 0 = the BVH walk of the render kernels (radiance_rays_kernel<.., true>); MIRT_RADIANCE_FLAT = the flat scan of the resident table,
 * the comparison build as MIRT_RAYS_FLAT is; MIRT_RADIANCE_SKY_HOSEK = the scene's Hosek blob, as MIRT_FLAG_SKY_HOSEK (MIRT_ERR_SKY
 * without a blob); MIRT_RADIANCE_SORT = the batch runs in an order the library derives on the device (radiance_rays_sorted_kernel<..>;
 * "sorted ray batches" below), same bytes in the same places, valid with every other flag; MIRT_RADIANCE_POOL = the pooled schedule
 * ("pooled radiance queries" below), a hint, same bytes in the same places, valid with every other flag; bits 3 and 5 are not assigned;
 * any other bit: MIRT_ERR_BAD_MODE.
 * MIRT_ERR_NULL_POINTER: ctx or params is null, or rays or the output is null with n_rays > 0;  MIRT_ERR_NO_SCENE: no scene, or not a
 * MIRT_SCENE_HBM one;  MIRT_ERR_SPP_ZERO, MIRT_ERR_SPP_RANGE: the rules of mirt_ctx_render;  MIRT_ERR_MATERIAL_INDEX / MIRT_ERR_TEXEL_RANGE:
 * exactly as a path-traced render call on that scene answers.  n_rays == 0 (after these checks): MIRT_OK without device work.  A refused
 * call queues nothing and writes nothing.
 *   mirt_ctx_trace_radiance          rays and records in HOST memory: copy, kernel, copy on the context's stream; blocking.  With
 *                                    MIRT_RADIANCE_ACCUMULATE it copies `out` to the device first.
 *   mirt_ctx_trace_radiance_device   pointers are memory of the context's device, 4-byte aligned: ONE kernel queued on `hip_stream` (NULL =
 *                                    the context's stream; hipStreamLegacy for the default stream), no host synchronisation; ordered
 *                                    against set_scene*, update_spheres* and set_spheres* the way ray queries are.
 * State is kept the way the ray queries keep it: neither the launch ring, MirtStats nor the accumulation is touched; mirt_ctx_last_kernel
 * names the kernel; mirt_ctx_synchronize and mirt_ctx_destroy wait for it; its time is mirt_ctx_trace_stats().kernel_ms (the counters
 * are 0). */
typedef struct MirtRadianceRay { float origin[3]; uint32_t stream; float direction[3]; uint32_t _pad; } MirtRadianceRay;   /* 32 B */
typedef struct MirtRadiance { uint64_t sum[3]; uint32_t samples; uint32_t _pad; } MirtRadiance;   /* 32 B */
typedef struct MirtRadianceParams { uint32_t spp, sample_begin, num_bounces, flags; uint64_t seed; } MirtRadianceParams;   /* 24 B */
enum { MIRT_RADIANCE_FLAT = 1u << 0, MIRT_RADIANCE_ACCUMULATE = 1u << 1, MIRT_RADIANCE_SKY_HOSEK = 1u << 2, MIRT_RADIANCE_SORT = 1u << 4 };   /* bit 3: unassigned */
enum { MIRT_RADIANCE_POOL = 1u << 6 };   /* bit 5: unassigned */
int mirt_ctx_trace_radiance(MirtContext* ctx, const MirtRadianceRay* rays, uint32_t n_rays, const MirtRadianceParams* params, MirtRadiance* out);
int mirt_ctx_trace_radiance_device(MirtContext* ctx, const void* d_rays, uint32_t n_rays, const MirtRadianceParams* params, void* d_out, void* hip_stream);

/* ---- pooled radiance queries: MIRT_RADIANCE_POOL ----
 * Without the flag lane = ray: a lane walks its ray's spp samples one after the other and in every sample the wave waits for its longest
 * path.  With it a wave owns 16 consecutive slots of the batch (slot k = ray k, or the k-th ray of the sorted order under
 * MIRT_RADIANCE_SORT) and keeps their 16 x spp (ray, sample) items in a wave-private pool of paths, as the pooled render of a
 * MIRT_SCENE_HBM scene (MIRT_FLAG_KERNEL_POOL) does with 16 pixels: a finished path's slot takes the next item at once.
 *   same bytes in the same places   the sums are exact integers, so the order in which the items are served cannot change them: the
 *                    records are those of the call without the flag, for every float bit pattern in a ray, and with every other flag
 *                    (_ACCUMULATE, _SKY_HOSEK, _SORT).  Errors, the n_rays == 0 rule and "a refused call queues and writes nothing" are
 *                    unchanged.  A record still depends on its ray, the params and the scene alone.
 *   a hint           like MIRT_FLAG_KERNEL_POOL.  The pooled kernel runs on the BVH build.  It does not run, and the call runs exactly as
 *                    without the flag (same kernel, same name in mirt_ctx_last_kernel), when MIRT_RADIANCE_FLAT is set, when
 *                    num_bounces > 255 (the pool's bounce counters are 8 bit), or when mirt_bvh_pool_plan of the resident tree's depth
 *                    gives slots == 0.  The geometry is mirt_bvh_pool_plan's for that depth and sky, as the pooled render's is.
 *   state            as for every radiance launch: the launch ring, MirtStats and the accumulation are untouched;
 *                    mirt_ctx_trace_stats().kernel_ms spans the launch, with the sort in front of it under _SORT; mirt_ctx_last_kernel
 *                    names radiance_rays_pool_kernel<THREADS,SLOTS,MINW,HOSEK,SORTED>.
 *   sharing          no context state is added beyond what radiance launches already write -- there is no dispenser word -- so pooled
 *                    launches need no ordering among themselves beyond what _SORT asks for its scratch. */

/* ---- sorted ray batches: MIRT_RAYS_SORT, MIRT_RADIANCE_SORT ----
 * Lane = ray and 64 consecutive records form a wave, so a batch that is not in a coherent order (probe grids, shuffled training rays)
 * walks the tree with waves whose lanes disagree.  With the flag the library computes a 31-bit code per ray on the device, sorts
 * (code, caller's index) with a stable radix sort and runs slot k of the query kernel on record order[k]; the records are neither moved
 * nor copied, every result lands at its ray's own position, and since a record depends on its ray alone the bytes are those of the call
 * without the flag, for every float bit pattern in a ray.  Errors, the n_rays == 0 rule and "a refused call queues and writes nothing"
 * are unchanged.  The order is ascending (code, caller's index) and depends on the rays and the resident tree's bounds alone.
 *   the code, float32, one IEEE operation at a time, no contraction (centre, radius: those of MirtBvhInfo):
 *     q(f, n)    = 0 if !(f > 0) (NaN included), n - 1 if f >= n, else (uint32_t)f (truncated)
 *     origin     inv = 16.0f / radius;  c[k] = q((o[k] - (centre[k] - radius)) * inv, 32): MIRT_RAY_SORT_ORIGIN_BITS = 5 bits per axis
 *     direction  octahedral: s = (|dx| + |dy|) + |dz|;  r = 1.0f / s;  u = dx * r;  v = dy * r;  if dz < 0, both from the old u, v:
 *                u' = (1 - |v|) * (u >= 0 ? 1 : -1), v' = (1 - |u|) * (v >= 0 ? 1 : -1);
 *                a = q(u * 128.0f + 128.0f, 256), b likewise from v: MIRT_RAY_SORT_DIRECTION_BITS = 8 bits per axis
 *     code       = morton3(c) << 16 | morton2(a, b);  bits 3j + 2, 3j + 1, 3j of morton3 = bit j of c[0], c[1], c[2];  bits 2j + 1, 2j of
 *                morton2 = bit j of a, b.  Every bit pattern has a code: an empty tree, a zero, infinite or NaN radius, a zero direction.
 *   Origin bits come first: probes differ by origin; a camera's rays share them and are ordered by direction.
 *   scratch      codes, order and the sort's storage belong to the context and only grow.  A call that must grow them waits for the
 *                device first; otherwise the device forms stay free of host synchronisation (code kernel, sort and query kernel are
 *                queued on `hip_stream`).  A failed allocation: MIRT_ERR_ALLOC, nothing queued, nothing written.  ALL sorted launches of a
 *                context share that scratch: the caller keeps them in order among themselves (one stream, or its own events), as for
 *                counting traces.  mirt_ctx_trace_stats().kernel_ms spans the code kernel through the query kernel.
 *   mirt_ray_sort_code          HOST ONLY, no device, no context: the code of one 32-byte record (MirtRay and MirtRadianceRay share what
 *                               it reads: origin at byte 0, direction at byte 16).  MIRT_ERR_NULL_POINTER for a null pointer.
 *   mirt_ctx_trace_order_read   blocking, for tests, like mirt_ctx_bvh_read: the permutation of the LAST sorted launch on the context,
 *                               order[k] = the caller's index of the ray that ran in slot k.  MIRT_ERR_NO_SCENE before the first sorted
 *                               launch, MIRT_ERR_OUT_BUFFER if len < its n_rays. */
#define MIRT_RAY_SORT_ORIGIN_BITS    5u
#define MIRT_RAY_SORT_DIRECTION_BITS 8u
int mirt_ray_sort_code(const float centre[3], float radius, const void* ray32, uint32_t* out_code);
int mirt_ctx_trace_order_read(MirtContext* ctx, uint32_t* order, size_t len);

/* Replace only the camera (`Layer::update_camera`, layer.rs:188-193; `Raytracer::set_render_params`,
 * mod.rs:353-388 — every interactive frame in the reference).  Host-side only: the camera travels by
 * value with each launch, so this neither copies to the device nor synchronises; launches already
 * queued keep their camera, the next render call uses the new one. */
int mirt_ctx_set_camera(MirtContext* ctx, const MirtGpuCamera* camera);

/* Render into HOST memory: kernel + D2H copy, blocking.  `out_rgba8` receives
 * mirt_params_out_rows() * width * 4 bytes.  This is the `set_data` replacement. */
int mirt_ctx_render(MirtContext* ctx, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);

/* Render into DEVICE memory `d_out_rgba8` (same layout) asynchronously on `hip_stream`
 * (a hipStream_t passed as void*; NULL = the context's own non-blocking stream; to run on the
 * default stream pass hipStreamLegacy, not 0).  No host sync: the caller orders later work on
 * the same stream (RCCL gather, D2H).  Used by bench.py and
 * the multi-GPU path so the framebuffer never leaves HBM before the collective. */
int mirt_ctx_render_device(MirtContext* ctx, const MirtParams* params, void* d_out_rgba8,
                           size_t out_len, void* hip_stream);

/* Name of the render kernel the LAST render call on this context launched (the schedule is chosen per call from
 * mode, spp, scene and flags), e.g. "render_pt_pool_kernel<256,112,6,false,false,3,false>" — the template
 * arguments as they appear in rocprofv3 kernel traces, without the `u` suffixes.  "" before the first render.
 * The pointer stays valid until the next render call or mirt_ctx_destroy. */
const char* mirt_ctx_last_kernel(const MirtContext* ctx);

/* Block until everything the context queued has finished. */
int mirt_ctx_synchronize(MirtContext* ctx);
/* Two streams of the context on DIFFERENT hardware queues, for hosts that keep two frames in flight -- a swap chain's double buffering:
 * queue frame k on stream k & 1 into framebuffer k & 1 (mirt_ctx_render_device) and the head of frame k + 1 fills the GPU while the tail
 * of frame k drains: 1080p, 2 spp 98.9 -> 83.9 us per frame; `Layer::set_data` at 800x600, 2 spp 12.8 -> 7.7 us.  index 0 is the context's
 * own stream (what a NULL hip_stream means), index 1 a stream of the device's highest priority, created on first use -- HIP keeps
 * hardware queues per priority, so the pair never shares one, which two streams of the caller's may (they then run one after the other).
 * *out_hip_stream is a hipStream_t owned by the context: pass it as `hip_stream`, wait on it with hipStreamSynchronize or
 * mirt_ctx_synchronize; it dies with the context.  Frames in flight must not share a framebuffer; mirt_ctx_accum_add calls stay ordered
 * among themselves (one stream).  MIRT_ERR_BAD_ROWS for index > 1. */
int mirt_ctx_frame_stream(MirtContext* ctx, uint32_t index, void** out_hip_stream);
/* Kernel timing on (the default) or off.  ON: every launch carries a start and an end event (on the kernel dispatch itself) and
 * mirt_ctx_get_stats reports kernel times.  OFF: a launch carries no event unless the context itself must learn that it has finished
 * (launches that take work units from the dispenser, counting launches): mirt_ctx_get_stats then counts launches but reports 0 ms for
 * them.  For hosts that queue frame after frame (the reference's render loop: `Raytracer::render_frame`, mod.rs:303-351;
 * `Layer::set_data` per resize): one `set_data` at the reference's operating point (800x600, 2 spp) takes 12.9 us per launch instead
 * of 17.9.  mirt_ctx_synchronize / mirt_ctx_set_scene / mirt_ctx_destroy still wait for such launches (through their streams). */
int mirt_ctx_set_timing(MirtContext* ctx, int enabled);
/* Stats of the last completed render call (synchronises the context first). */
int mirt_ctx_get_stats(MirtContext* ctx, MirtStats* out);

/* ---- progressive accumulation: what `RenderProgress::next_frame` (mod.rs:615-679) and the f32
 * image buffer of fsMain (wgsl:61-80) do across frames.  The context owns one accumulation buffer of
 * EXACT 64-bit fixed-point sums (3 per pixel, 2^-20 units), so frames add up bit-identically to
 * a single launch with the total sample count.  Path-traced mode only. ---- */

/* (Re)size the buffer for the rows `params` selects and clear it (`clear_accumulated_samples`). */
int mirt_ctx_accum_reset(MirtContext* ctx, const MirtParams* params);
/* Render params->spp further samples of every pixel (samples accumulated so far .. +spp of the RNG
 * stream; params->sample_begin is ignored) and add them to the buffer.  Asynchronous on `hip_stream`
 * (NULL = the context's stream). */
int mirt_ctx_accum_add(MirtContext* ctx, const MirtParams* params, void* hip_stream);
/* Samples per pixel accumulated since the last reset (`accumulated_samples_per_pixel`). */
uint32_t mirt_ctx_accum_samples(const MirtContext* ctx);
/* Resolve the buffer (mean over the accumulated samples, tone curves per params->flags) into
 * host memory, RGBA8; blocking.  Ordered after every mirt_ctx_accum_add issued so far, whatever
 * stream it was queued on (so is mirt_ctx_accum_read). */
int mirt_ctx_accum_resolve(MirtContext* ctx, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);
/* Copy the raw sums to the host: pixels x 3 uint64 (the fp32-intermediate view used by tests). */
int mirt_ctx_accum_read(MirtContext* ctx, uint64_t* out_sums, size_t out_len_u64);
/* ONE progressive frame, the shape of fsMain (wgsl:61-80; `Raytracer::render_frame`, mod.rs:303-351), into DEVICE memory `d_out_rgba8`
 * (the layout of mirt_ctx_render_device), asynchronously on `hip_stream` (NULL = the context's stream), with no host synchronisation:
 *   params->spp >= 1   ONE kernel launch: renders spp further samples of every pixel (the rules of mirt_ctx_accum_add: sample_begin is
 *                      ignored, frame_spp / frame_begin are checked the same way), adds them to the sums and, in the same pass, writes
 *                      the resolve of the UPDATED sums over all samples accumulated, tone curves per params->flags.  The schedule is
 *                      the one mirt_ctx_accum_add would take; the kernel is its progressive-frame build (mirt_ctx_last_kernel:
 *                      "render_pt_strip_frame_kernel<...>", "render_pt_stream_frame_kernel<...>", "render_pt_pool_frame_kernel<...>",
 *                      "render_pt_pool_tile_frame_kernel<...>", "render_pt_hbm_frame_kernel<...>").  The bytes are those of
 *                      mirt_ctx_accum_add followed by mirt_ctx_accum_resolve; the sums are those of mirt_ctx_accum_add.
 *   params->spp == 0   adds nothing: resolve_accum_kernel writes the mean of what is there -- the reference's frame once the accumulation
 *                      is complete (mod.rs:350).  MIRT_ERR_NO_SCENE if nothing has been accumulated.  Only the frame calls accept spp == 0.
 * Errors as mirt_ctx_accum_add, plus MIRT_ERR_NULL_POINTER / MIRT_ERR_OUT_BUFFER for the output; a refused call leaves sums and count
 * untouched.  A frame reads the sums the previous one wrote: consecutive frames on DIFFERENT streams (two frames in flight on
 * mirt_ctx_frame_stream, into two framebuffers) are ordered by the library with an event wait on the device, whether they add or only
 * read (spp == 0): the frames form one chain.  (hipStreamLegacy takes no part in event waits: the host waits for it instead.)  Later
 * mirt_ctx_accum_resolve / _read / _reset calls are ordered after a frame exactly as after a mirt_ctx_accum_add on that stream.
 * mirt_ctx_accum_add itself waits for nothing: an add that follows a frame on another stream is ordered by the caller, as adds among
 * themselves are. */
int mirt_ctx_accum_frame_device(MirtContext* ctx, const MirtParams* params, void* d_out_rgba8, size_t out_len, void* hip_stream);
/* The same frame into HOST memory: the context's own device buffer, one D2H copy, blocking -- as mirt_ctx_render relates to
 * mirt_ctx_render_device.  For hosts without HIP. */
int mirt_ctx_accum_frame(MirtContext* ctx, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);

/* ---- adaptive sampling for progressive frames of a MIRT_SCENE_HBM scene ----
 * mirt_ctx_accum_add gives every pixel the same number of samples.  Here the context keeps one 64-byte record per pixel and a step
 * samples only the pixels that have not converged: sky, ground and plain lambertians settle after a handful of samples, glass, metal
 * reflections and defocused edges take hundreds.  Everything is integer: a pixel's sample s depends on (pixel index, s, seed) alone, so
 * a pixel's sums after n samples are the same whatever the other pixels received, and the whole loop -- which pixels a step samples,
 * and every sum -- has ONE right answer.
 *   the record       sum[k] = the sum of to_fixed(radiance[k]) over the pixel's samples 0 .. samples - 1, the units of the accumulation
 *                    buffer (2^-20, each sample clamped to [0, 4096)); even[k] = the same sum over the samples whose index is even; the
 *                    pads are written as 0.  The records are a buffer of their own: the accumulation API neither sees nor disturbs it.
 *   the rule         exact, in integers of unlimited width (128 bits suffice for EVERY bit pattern of a record), per pixel, no neighbourhood:
 *                      e = sum over k of |2 * even[k] - sum[k]|      m = sum over k of sum[k]      n = samples
 *                      converged  <=>  n >= 2  and  e * 2^16 <= tolerance * (m + n * MIRT_ADAPT_FLOOR)
 *                      active     <=>  n < max_samples  and  (n < min_samples  or  not converged)
 *                    `tolerance` is a relative error in units of 2^-16: the difference of the even and the odd half against the mean.
 *                    MIRT_ADAPT_FLOOR is 0.125 of radiance per sample, summed over the channels: it keeps dark, noisy pixels from
 *                    taking every sample.  mirt_adapt_active is that rule for one record, HOST ONLY (no device, no context; *out = 1 or 0;
 *                    MIRT_ERR_NULL_POINTER for a null pointer): the device evaluates the same function, so the two agree on every record.
 *   a step           two stages on `hip_stream` (NULL = the context's stream), no host synchronisation.  Select: the rule for every
 *                    record (adapt_select_kernel), the indices of the active records in ASCENDING order into a list in device memory
 *                    and their count into a device word (a block scan: adapt_scan_kernel, adapt_compact_kernel); the same stage adds
 *                    count * spp to a 64-bit device counter.  Render (adapt_pixels_kernel<HOSEK,BVH>: lane = list entry, one wave per block,
 *                    the grid sized for all pixels, blocks beyond the count return at once): every listed pixel receives exactly
 *                    params->spp further samples, indices samples .. samples + spp - 1 of its own stream -- the renderer's sample for the
 *                    pixel's ABSOLUTE index x + y * width, whatever band the buffer covers.  A pixel may therefore overshoot max_samples
 *                    by less than spp.  A record's place is the pixel's place in the compact band (row-major, mirt_params_out_row_index).
 *   of MirtParams    a step reads width, height, the row fields, spp, num_bounces, seed and of flags MIRT_FLAG_SKY_HOSEK and
 *                    MIRT_FLAG_NO_GRID (the flat scan of the table, the comparison build); sample_begin is ignored, schedule hints
 *                    (MIRT_FLAG_KERNEL_STRIP / _POOL, _TEXEL_TILES, _FAST_MATH) are ignored; the resolve flags matter to the resolve only.
 *   errors of a step MIRT_ERR_NULL_POINTER: ctx, params or adapt is null;  MIRT_ERR_NO_SCENE: no scene, or not a MIRT_SCENE_HBM one;
 *                    MIRT_ERR_BAD_MODE: mode is not MIRT_MODE_PT, a bit of adapt->flags other than MIRT_ADAPT_POOL, or a counting flag (MIRT_FLAG_COUNT_WORK, _COUNT_GRID);
 *                    MIRT_ERR_FRAME_SPP: frame_spp != 0 (a pixel's samples must be independent);  MIRT_ERR_SPP_RANGE: spp is odd (the two
 *                    halves grow together), or max_samples > MIRT_MAX_SPP_PER_CALL;  MIRT_ERR_OUT_BUFFER: no buffer, or another width or
 *                    row count than the reset's;  every other check and code is that of a path-traced render on that scene.  A refused
 *                    call queues nothing and writes nothing.
 *   ordering         a step is ordered against set_scene*, update_spheres* and set_spheres* the way radiance queries are (they wait for
 *                    the device).  Steps, resolves, reads and writes of one context are ordered among themselves by the caller (one
 *                    stream); the blocking calls wait for the last step first.  The launch ring, MirtStats and the accumulation are
 *                    untouched; mirt_ctx_last_kernel names the render kernel; mirt_ctx_synchronize and mirt_ctx_destroy wait for a step.
 *   mirt_ctx_adapt_reset           sizes the buffer for the rows `params` selects and clears it, records, counters and list: the rules of
 *                                  mirt_ctx_accum_reset (bands and tile partitions included).  The list, its count and the select
 *                                  stage's storage are sized here, belong to the context and only grow: a step allocates nothing.
 *   mirt_ctx_adapt_step_device     one step, as above.
 *   mirt_ctx_adapt_resolve_device  adapt_resolve_kernel: per pixel the resolve of sum[k] over ITS samples, tone curves per params->flags,
 *                                  RGBA8 into device memory on `hip_stream`; a pixel with samples == 0 is black, A = 255.  MIRT_ERR_NO_SCENE
 *                                  before the first step since the reset, MIRT_ERR_OUT_BUFFER if out_len < pixels * 4.
 *   mirt_ctx_adapt_resolve         the same into HOST memory; blocking.
 *   mirt_ctx_adapt_read / _write   blocking copies of the records to / from the host (len in records, at least / exactly the buffer's
 *                                  pixels: MIRT_ERR_OUT_BUFFER otherwise; MIRT_ERR_NO_SCENE without a buffer): checkpoints and tests.
 *   mirt_ctx_adapt_list_read       blocking: the list of the LAST step and its count, like mirt_ctx_trace_order_read.  MIRT_ERR_NO_SCENE before
 *                                  the first step since the reset, MIRT_ERR_OUT_BUFFER if len < count (*count is set all the same).
 *   mirt_ctx_adapt_stats           blocking: pixels of the buffer, `active` = the count of the last step, steps and samples added since the
 *                                  reset (the device counter), kernel_ms of the last step, select through render (0 with timing off).
 * A stopping rule makes the mean of a stopped pixel slightly biased, and a moved world or camera makes the records stale: reset. */
typedef struct MirtAdaptPixel { uint64_t sum[3]; uint64_t even[3]; uint32_t samples; uint32_t _pad0; uint64_t _pad1; } MirtAdaptPixel; /* 64 B */
typedef struct MirtAdaptParams { uint32_t min_samples, max_samples, tolerance, flags; } MirtAdaptParams;                               /* 16 B */
typedef struct MirtAdaptStats { uint64_t pixels, total_samples; uint32_t active, steps; double kernel_ms; } MirtAdaptStats;            /* 32 B */
#define MIRT_ADAPT_FLOOR (1u << 17)
enum { MIRT_ADAPT_POOL = 1u << 1 };   /* MirtAdaptParams.flags; bit 0: unassigned */
int mirt_adapt_active(const MirtAdaptPixel* pixel, const MirtAdaptParams* adapt, uint32_t* out);
int mirt_ctx_adapt_reset(MirtContext* ctx, const MirtParams* params);
int mirt_ctx_adapt_step_device(MirtContext* ctx, const MirtParams* params, const MirtAdaptParams* adapt, void* hip_stream);
int mirt_ctx_adapt_resolve_device(MirtContext* ctx, const MirtParams* params, void* d_out_rgba8, size_t out_len, void* hip_stream);
int mirt_ctx_adapt_resolve(MirtContext* ctx, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);
int mirt_ctx_adapt_read(MirtContext* ctx, MirtAdaptPixel* out, size_t len);
int mirt_ctx_adapt_write(MirtContext* ctx, const MirtAdaptPixel* in, size_t len);
int mirt_ctx_adapt_list_read(MirtContext* ctx, uint32_t* list, size_t len, uint32_t* count);
int mirt_ctx_adapt_stats(MirtContext* ctx, MirtAdaptStats* out);

/* ---- pooled adaptive steps: MIRT_ADAPT_POOL in MirtAdaptParams.flags ----
 * Without the flag lane = list entry: a lane walks its pixel's spp samples one after the other, in every sample the wave waits for its
 * longest path, and a late, short list is a handful of waves on a device that holds thousands.  With it a wave owns 16 consecutive
 * entries of the list and deals their 16 x spp (pixel, sample) items to a wave-private pool of paths, as MIRT_RADIANCE_POOL does with
 * 16 rays: a finished path's slot takes the next item at once.
 *   same bytes in the same places   the sums are exact integers, so after a step with the flag the list and its count, the 64-bit
 *                    sample counter and all 64 bytes of every record (pads written as 0, unlisted records untouched) equal those of
 *                    the same step without it, for every record mirt_ctx_adapt_write can put there.  Errors are unchanged, except that
 *                    MIRT_ADAPT_POOL is a known bit; a refused call queues nothing and writes nothing.
 *   a hint           like MIRT_FLAG_KERNEL_POOL and MIRT_RADIANCE_POOL.  The pooled kernel runs on the BVH build.  The step runs exactly
 *                    as without the flag (same kernel, same name in mirt_ctx_last_kernel) when MIRT_FLAG_NO_GRID is set, when
 *                    num_bounces > 255 (the pool's bounce counters are 8 bit), or when mirt_adapt_pool_plan of the resident tree's
 *                    depth gives slots == 0.
 *   state            as for every adaptive step: one event pair around select through render; the launch ring, MirtStats and the
 *                    accumulation untouched; steps of one context ordered by the caller.  There is no dispenser word.
 *                    mirt_ctx_last_kernel names adapt_pixels_pool_kernel<THREADS,SLOTS,MINW,HOSEK>.
 *   mirt_adapt_pool_plan   HOST-ONLY, the function the launch itself uses: the arguments, struct, rule and errors of mirt_bvh_pool_plan.
 *                    Beside the 16 x 3 sums a wave's pool keeps the 16 x 3 sums of the even-indexed samples (384 bytes) and
 *                    {place in the band, samples so far} of its 16 entries (128 bytes):
 *                      lds_bytes_per_block = 96 (+ 144) + threads / 64 * (50 * slots + 896 + 256 * max_depth). */
int mirt_adapt_pool_plan(uint32_t max_depth, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtBvhPoolPlan* out);

/* ---- adaptive runs: a whole loop per call, step sizes chosen on the device ----
 * mirt_ctx_adapt_run_device queues run->max_steps adaptive steps in order on hip_stream (NULL = the context's), with no host
 * synchronisation, no allocation and no read of the count in between.  Step j selects exactly as mirt_ctx_adapt_step_device does (the
 * same rule, the ascending list, the count); its scan stage then chooses the step's sample count ON THE DEVICE, from the count it has
 * just summed, by an integer rule:
 *   the step size    base = params->spp (even, at least 2, as for a step); cap = run->max_spp, 0 meaning base.  spp_j = 0 when count_j is 0,
 *                    otherwise base << k with k the smallest k >= 0 for which count_j * (base << k) >= run->min_items or
 *                    (base << k) == cap; the product is 64 bit.  min_items == 0 never grows.  mirt_adapt_run_spp is that rule for one
 *                    count, HOST ONLY (no device, no context; it is the function the scan stage's thread runs: csrc/mirt_adapt_rule.h).
 *                    Its errors: MIRT_ERR_NULL_POINTER (run or out), MIRT_ERR_BAD_MODE (run->flags != 0), MIRT_ERR_SPP_RANGE (spp is 0,
 *                    odd or above MIRT_MAX_SPP_PER_CALL, or max_spp as below).
 *   a step of a run  every listed pixel receives samples n .. n + spp_j - 1 of ITS stream: `sum` grows by every sample, `even` by the
 *                    samples whose OWN index is even, samples = n + spp_j, the pads are written as 0; the 64-bit counter grows by
 *                    count_j * spp_j, and entry j of a run log in device memory receives {count_j, spp_j}.  A pixel may overshoot
 *                    max_samples by less than spp_j <= cap: the caller bounds that through max_spp.  The render kernels are builds of
 *                    their own, adapt_pixels_run_kernel<HOSEK,BVH> and adapt_pixels_pool_run_kernel<THREADS,SLOTS,MINW,HOSEK>, which read
 *                    spp_j as a wave-uniform word next to the count.  A run of max_steps = 1, min_items = 0, max_spp = 0 leaves the bytes
 *                    of one mirt_ctx_adapt_step_device.
 *   empty steps      once a step lists nothing every later step of the run lists nothing either (the records did not change).  Such
 *                    steps are queued and run as empty steps do today -- the select stage runs, the render stage's blocks return at once
 *                    -- and leave records, list, count (0) and counter as they are; they log {0, 0}.
 *   state            mirt_ctx_adapt_list_read and mirt_ctx_adapt_stats().active describe the run's LAST step; steps grows by max_steps.
 *                    One event pair around the whole run: kernel_ms spans it.  mirt_ctx_last_kernel names the run's render kernel.  The
 *                    launch ring, MirtStats and the accumulation are untouched; ordering against set_scene*, update_spheres*,
 *                    set_spheres*, resolves, reads and writes is that of a step.  The log (MIRT_ADAPT_RUN_MAX_STEPS entries) is part of the
 *                    buffer mirt_ctx_adapt_reset sizes and clears.
 *   honoured         MIRT_ADAPT_POOL in adapt->flags (the same hint, the same fall-backs), MIRT_FLAG_SKY_HOSEK, MIRT_FLAG_NO_GRID, bands
 *                    and tile partitions.
 *   errors           MIRT_ERR_NULL_POINTER: ctx, params, adapt or run is null; then every check and code of a step, in a step's order; then
 *                    MIRT_ERR_BAD_MODE: run->flags != 0;  MIRT_ERR_BAD_ROWS: max_steps is 0 or above MIRT_ADAPT_RUN_MAX_STEPS;
 *                    MIRT_ERR_SPP_RANGE: max_spp is neither 0 nor params->spp << m, or exceeds MIRT_MAX_SPP_PER_CALL.  A refused call queues
 *                    nothing and writes nothing.
 *   mirt_ctx_adapt_run_read   blocking, for tests and hosts: the log of the LAST run, entries 0 .. max_steps - 1 of it, and *n_steps =
 *                    its max_steps.  MIRT_ERR_NO_SCENE before the first run since the reset; MIRT_ERR_OUT_BUFFER if len < that max_steps
 *                    (*n_steps is set all the same). */
typedef struct MirtAdaptRun     { uint32_t max_steps, min_items, max_spp, flags; } MirtAdaptRun;      /* 16 B */
typedef struct MirtAdaptRunStep { uint32_t count, spp; } MirtAdaptRunStep;                           /*  8 B */
#define MIRT_ADAPT_RUN_MAX_STEPS 256u
int mirt_adapt_run_spp(uint32_t count, uint32_t spp, const MirtAdaptRun* run, uint32_t* out);
int mirt_ctx_adapt_run_device(MirtContext* ctx, const MirtParams* params, const MirtAdaptParams* adapt, const MirtAdaptRun* run, void* hip_stream);
int mirt_ctx_adapt_run_read(MirtContext* ctx, MirtAdaptRunStep* out, size_t len, uint32_t* n_steps);

/* ---- adaptive steps on a scene that lives in LDS: MIRT_ADAPT_LDS in MirtAdaptParams.flags ----
 * Without the flag an adaptive step needs a MIRT_SCENE_HBM scene.  With it mirt_ctx_adapt_step_device and mirt_ctx_adapt_run_device also
 * accept a context whose scene lives in LDS (mirt_ctx_set_scene, or mirt_ctx_set_scene_ex with flags 0), where it stays: the select
 * stage is unchanged, the render stage is adapt_pixels_lds_kernel<HOSEK,GRID> (a run: adapt_pixels_lds_run_kernel<HOSEK,GRID>).
 *   same bytes       after a step or run with the flag on an LDS scene the list and its count, the 64-bit sample counter, the run log and
 *                    all 64 bytes of every record (pads written as 0, unlisted records untouched) equal what the same call leaves on a
 *                    context that holds the same world as a MIRT_SCENE_HBM scene: integer sums of the same samples.
 *   an HBM scene     ignores the flag: same kernel, same name in mirt_ctx_last_kernel, same bytes as without it.
 *   an LDS scene     without the flag: MIRT_ERR_NO_SCENE, as ever.  With it MIRT_ADAPT_POOL is a hint that is ignored (there is no pooled
 *                    LDS build); any other bit of adapt->flags is MIRT_ERR_BAD_MODE.  Every other check and code of a step, in a step's
 *                    order; last of all the layout, below.  A refused call queues nothing and writes nothing.
 *   the layout       the scene's uniform grid when it has one (mirt_grid_plan) and MIRT_FLAG_NO_GRID is not set; otherwise the flat
 *                    layout if the scene fits it; otherwise MIRT_ERR_SCENE_TOO_LARGE, the code a render with MIRT_FLAG_NO_GRID gives on
 *                    such a scene.  MIRT_FLAG_SKY_HOSEK is honoured; schedule hints are ignored.
 *   the kernel       blocks of 256 threads whose four waves share one staged scene, in a PERSISTENT grid of
 *                    min(ceil(pixels / 256), CUs x blocks_per_cu) blocks, blocks_per_cu the smaller of mirt_adapt_lds_plan's and the
 *                    occupancy query's answer.  A unit is 64 >> g consecutive list entries, their spp samples dealt to 1 << g groups of
 *                    lanes; waves stride over the units.  g is chosen ON THE DEVICE from the count:  g_cap = min(2, trailing zero bits
 *                    of spp);  g = the smallest of 0 .. g_cap with ceil(count / (64 >> g)) >= grid_waves = blocks x 4, else g_cap; 0 for
 *                    an empty list.  In a run spp is the step's spp_j.  A short late list is then four times as many waves.
 *   state            as for every adaptive step: one event pair; the launch ring, MirtStats and the accumulation untouched.
 *   mirt_adapt_lds_plan    HOST-ONLY, the function the launch itself uses.  grid_bytes = MirtGridPlan.blob_bytes of the scene, 0 for the
 *                    flat layout; lds_bytes_per_cu == 0 means gfx950's 163 840.  threads = 256; grid = 1 for the grid layout, else 0;
 *                      lds_bytes_per_block = 96 (+ 144 with hosek) + (grid_bytes ? grid_bytes : 32 * n_spheres + 48 * n_materials)
 *                      blocks_per_cu       = min(8, lds_bytes_per_cu / lds_bytes_per_block)
 *                    A layout the render launches refuse -- with the sky's 144 bytes counted, as mirt_ctx_set_scene counts them: more
 *                    than 122 880 bytes, or a grid over more than 4 095 spheres -- or one that exceeds lds_bytes_per_cu gives all
 *                    fields 0.  A large flat scene gets one or two blocks per CU: four or eight waves.  That is documented, not tuned.
 *                    MIRT_ERR_NULL_POINTER for a null `out`.
 *   mirt_adapt_lds_groups  HOST-ONLY: the rule for g above, for one count (the function every wave runs: csrc/mirt_adapt_rule.h).
 *                    MIRT_ERR_NULL_POINTER: out_log2 is null;  MIRT_ERR_SPP_RANGE: spp is 0, odd or above MIRT_MAX_SPP_PER_CALL;
 *                    MIRT_ERR_BAD_ROWS: grid_waves is 0.
 * Knobs, read once in mirt_ctx_create (tests, A/B runs): MIRT_ADAPT_LDS_BLOCKS=n launches at most n blocks; MIRT_ADAPT_LDS_GROUPS=1|2|3
 * forces g = 0|1|2, still capped by spp. */
enum { MIRT_ADAPT_LDS = 1u << 3 };    /* MirtAdaptParams.flags; bit 2: unassigned */
typedef struct MirtAdaptLdsPlan { uint32_t threads, grid, lds_bytes_per_block, blocks_per_cu; } MirtAdaptLdsPlan;   /* 16 B */
int mirt_adapt_lds_plan(uint32_t n_spheres, uint32_t n_materials, uint32_t grid_bytes, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtAdaptLdsPlan* out);
int mirt_adapt_lds_groups(uint32_t count, uint32_t spp, uint32_t grid_waves, uint32_t* out_log2);

/* ---- ray, feature and radiance queries on a scene that lives in LDS: MIRT_QUERY_LDS ----
 * One bit, accepted in three flag words: the `flags` of mirt_ctx_trace_rays*, the `flags` of mirt_ctx_render_features* and
 * MirtRadianceParams.flags.  Without it those calls answer MIRT_ERR_NO_SCENE on a scene that is not a MIRT_SCENE_HBM one, as ever.
 *   an HBM scene     ignores the flag: the kernel, the name in mirt_ctx_last_kernel and the bytes are those of the call without it.
 *   an LDS scene     every other check keeps its place and its code; the layout is checked last.  The call uses the scene's uniform
 *                    grid when it has one and the family's _FLAT bit (MIRT_RAYS_FLAT, MIRT_FEATURES_FLAT, MIRT_RADIANCE_FLAT) is not
 *                    set; otherwise the flat tables, if the scene fits them; otherwise it answers MIRT_ERR_SCENE_TOO_LARGE, the code a
 *                    render with MIRT_FLAG_NO_GRID gives on a grid-only scene.  A refused call queues nothing and writes nothing.
 *   same bytes       every record of every family, for every float bit pattern in a ray, equals the record of the same call without
 *                    the flag on a context that holds the same world as a MIRT_SCENE_HBM scene (either tree builder), whose bytes
 *                    are in turn those of its _FLAT build.  MIRT_RAYS_ANY_HIT, MIRT_RAYS_COUNT, MIRT_RADIANCE_ACCUMULATE and
 *                    MIRT_RADIANCE_SKY_HOSEK are honoured.
 *   schedule hints   MIRT_RAYS_SORT, MIRT_RADIANCE_SORT and MIRT_RADIANCE_POOL are accepted and ignored on an LDS scene (there is no
 *                    tree to take bounds from and no pooled LDS query build); the bytes are the same by those flags' own contracts.
 *                    Such a call is no sorted launch: mirt_ctx_trace_order_read keeps describing the last launch that really sorted.
 *   counters         under MIRT_RAYS_COUNT, flat layout: rays, sphere_tests, roots and hits are those of MIRT_RAYS_FLAT |
 *                    MIRT_RAYS_COUNT on the HBM twin, nodes and wave_nodes 0.  Grid: rays and hits are the twin's, sphere_tests and
 *                    roots count what the lanes really perform, nodes counts grid cells visited summed over lanes, wave_nodes
 *                    cell-loop iterations summed over waves.
 *   state            as for every query: the launch ring, MirtStats and the accumulation are untouched, mirt_ctx_trace_stats().kernel_ms
 *                    spans the kernel, mirt_ctx_synchronize and mirt_ctx_destroy wait for it.  mirt_ctx_last_kernel names
 *                    trace_rays_lds_kernel<grid,any,count>, feature_frame_lds_kernel<grid> or radiance_rays_lds_kernel<hosek,grid>.
 *   geometry         mirt_adapt_lds_plan's for the layout (hosek = 0 for ray and feature queries, which stage no sky): 256-thread
 *                    blocks, a persistent grid of min(ceil(items / 256), CUs x blocks per CU), the blocks per CU the smaller of the
 *                    plan's bound and the kernel's occupancy.  MIRT_QUERY_LDS_BLOCKS=n (read once in mirt_ctx_create; tests, A/B runs)
 *                    launches at most n blocks. */
enum { MIRT_QUERY_LDS = 1u << 8 };

/* ---- denoise a progressive or an adaptive frame on the device: an edge-avoiding a-trous filter ----
 * Filters the mean of the context's exact sums with the caller's feature frame as guide.  No scene is read: the call works on HBM and
 * LDS scenes alike, and on a context whose scene has been replaced since.  It is a fixed spatial filter, not a learned denoiser.
 *   source       MIRT_DENOISE_SRC_ACCUM: the accumulation buffer, sum[3] per pixel, n = mirt_ctx_accum_samples for every pixel;
 *                MIRT_DENOISE_SRC_ADAPT: the adaptive records, sum[3] and n = samples per pixel.
 *   guides       one MirtFeaturePixel per pixel of the same compact band, device memory (the _device form) or host memory: what
 *                mirt_ctx_render_features* wrote for the same width, height and rows.  4-byte aligned; every bit pattern is defined.
 *   params       read: width, height and the row fields (checked against the source's reset), MIRT_FLAG_NO_TONEMAP and
 *                MIRT_FLAG_NO_SRGB of flags.  Nothing else.
 *   output       row-major over the band.  RGBA8 with A = 255, 4 bytes per pixel; with MIRT_DENOISE_OUT_F32 {r, g, b, 1.0f} as
 *                float32, 16 bytes per pixel: the linear mean before the tone curves.
 *   arithmetic   float32, every operation a single IEEE operation in the order written, no contraction.  p a pixel, k a channel,
 *                W x R the band.
 *                  m[k]   = (float)((double)sum[k] / ((double)n * 1048576.0)), 0 for n == 0       (the mean of the resolves)
 *                  den[k] = albedo[k] if sphere != MIRT_RAY_MISS and 0.015625f <= albedo[k] <= 64.0f, else 1.0f
 *                  c[k]   = m[k] / den[k]
 *                  level i = 0 .. levels - 1, s = 1 << i:  inv_i = 1.0f / (sg * sg), sg = sigma_colour * 2^-i (host, float32);
 *                    taps q = p + s * (dx, dy), dy = -2..2 outer, dx = -2..2 inner, a tap outside [0, W) x [0, R) skipped;
 *                    kern = b[dx + 2] * b[dy + 2], b = {1, 4, 6, 4, 1}; the centre tap has w = 36; every other tap
 *                      wg = 1 if both sphere fields are MIRT_RAY_MISS, 0 if they differ, otherwise x = (n_p[0] * n_q[0] +
 *                           n_p[1] * n_q[1]) + n_p[2] * n_q[2], x = (x > 0) ? ((x < 1) ? x : 1) : 0, x = x * x normal_log2 times
 *                      wc = 1 if sigma_colour == 0, otherwise d[k] = c_p[k] - c_q[k], d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2],
 *                           wc = exp(-(d2 * inv_i)) with mirt-math's exp
 *                      w  = (kern * wg) * wc
 *                    wsum = wsum + w, acc[k] = acc[k] + w * c_q[k], both from +0 in tap order; c'[k] = acc[k] / wsum
 *                  r[k]   = c[k] * den[k];  F32 stores {r[0], r[1], r[2], 1.0f}; RGBA8 stores the resolve of the 2^-20 fixed-point
 *                           value of r[k] at one sample, per params->flags
 *   errors       in this order.  MIRT_ERR_NULL_POINTER: ctx, params, denoise, guides or out is null.  MIRT_ERR_BAD_MODE: unknown
 *                source or flag bit, levels outside 1..8, normal_log2 above 8, sigma_colour negative or NaN, or positive with an
 *                inv_i that is not finite and positive.  MIRT_ERR_BAD_ROWS: a tile partition (n_parts > 1 with tile_rows != 0): its
 *                compact rows are not neighbours in the image.  MIRT_ERR_OUT_BUFFER: no buffer of that source, another width or row
 *                count than its reset, guides_len < pixels * 32, out_len too small.  MIRT_ERR_NO_SCENE: nothing accumulated, or no
 *                adaptive step since the reset (the codes of the two resolves).  MIRT_ERR_ALLOC: scratch could not be grown.  A
 *                refused call queues nothing and writes nothing.
 *   state        the sums, records, guides, launch ring, MirtStats and sample counts are untouched.  mirt_ctx_trace_stats().kernel_ms
 *                spans the first through the last kernel, mirt_ctx_last_kernel names the a-trous kernel, mirt_ctx_synchronize and
 *                mirt_ctx_destroy wait for it.
 *   scratch      two colour planes and one guide plane, 16 bytes per pixel each; the context's, grows only.  A call that must grow it
 *                waits for the device first.  All denoise launches of a context share it: the caller keeps them in order among
 *                themselves, as for sorted launches.
 *   ordering     an ACCUM denoise is a reading link of the progressive frame chain, exactly as mirt_ctx_accum_frame_device with
 *                spp == 0: ordered after the last frame on whatever stream, and mirt_ctx_accum_reset / _resolve / _read wait for it.
 *                An ADAPT denoise is ordered by the caller against steps, like mirt_ctx_adapt_resolve_device.  The _device form has
 *                no host synchronisation (unless the scratch grows). */
typedef struct MirtDenoiseParams { uint32_t source, levels, normal_log2, flags; float sigma_colour; uint32_t _pad[3]; } MirtDenoiseParams; /* 32 B; _pad is not read */
enum { MIRT_DENOISE_SRC_ACCUM = 0, MIRT_DENOISE_SRC_ADAPT = 1 };   /* source */
enum { MIRT_DENOISE_OUT_F32 = 1u << 0 };                            /* flags  */
int mirt_ctx_denoise_device(MirtContext* ctx, const MirtParams* params, const MirtDenoiseParams* denoise, const void* d_guides, size_t guides_len,
                            void* d_out, size_t out_len, void* hip_stream);
int mirt_ctx_denoise(MirtContext* ctx, const MirtParams* params, const MirtDenoiseParams* denoise, const MirtFeaturePixel* guides, size_t guides_len,
                     void* out, size_t out_len);    /* host memory; blocking */

/* ---- carry a denoised frame across camera motion: temporal reprojection by first-hit depth and id ----
 * Takes the previous frame's result to this frame's pixels and blends it with this frame's colour.  No scene, no accumulation and no
 * context state is read: the call works on HBM and LDS scenes alike and with no scene set at all.
 *   params       read: width, height, the row fields, MIRT_FLAG_NO_TONEMAP and MIRT_FLAG_NO_SRGB of flags.  Nothing else.  Both frames
 *                have this width, height and band; the host drops its history on a resize.
 *   frames       all device pointers (the _device form) or all host pointers, 4-byte aligned, row-major over the compact band:
 *                  colour        float32 x 4 per pixel: this frame, {r, g, b, ignored} -- what MIRT_DENOISE_OUT_F32 wrote
 *                  guides        MirtFeaturePixel per pixel: this frame, taken with `current`
 *                  prev_colour   float32 x 4: {r, g, b, history length} -- the `out` of the previous call, or a denoise output (length 1)
 *                  prev_guides   MirtFeaturePixel: the previous frame, taken with `previous`
 *                  out           float32 x 4: {r, g, b, new history length}
 *                  out_rgba8     nullable: the same pixel through the 2^-20 fixed-point value and the resolve at one sample per
 *                                params->flags, A = 255
 *                  pixels        records every non-null buffer holds; >= rows * width
 *   arithmetic   float32, every operation one IEEE operation in the order written, no contraction; the only fused operations are the
 *                fmaf written out.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  For pixel (x, y) of the band (y the image row, compact row
 *                y - row_begin, p its compact index):
 *                  (o, d)  = the centre ray of (x, y) under `current`, exactly as mirt_camera_pixel_ray
 *                  g       = guides[p]; hit = g.sphere != MIRT_RAY_MISS
 *                  rel[k]  = hit ? fmaf(g.t, d[k], o[k]) - previous.eye[k] : d[k]           (a miss is a direction: rotation only)
 *                  a[k]    = previous.lower_left_corner[k] - previous.eye[k];  H = previous.horizontal;  V = previous.vertical
 *                  n       = (H1*V2 - H2*V1, H2*V0 - H0*V2, H0*V1 - H1*V0)
 *                  s       = dot(rel, n) / dot(a, n)                                (the ray parameter of the point in the previous frame)
 *                  q[k]    = rel[k] / s - a[k];  pu = dot(q, H) / dot(H, H);  pv = dot(q, V) / dot(V, V)
 *                  fx      = pu * (float)width - 0.5f;  fy = (1.0f - pv) * (float)height - 0.5f
 *                  ok      = s > 0 && s < +inf && fx > -1 && fx < (float)width && fy > -1 && fy < (float)height     (false on NaN)
 *                  flx = floorf(fx), ix = (int32)flx, wx = fx - flx; likewise fly, iy, wy
 *                  taps    dy = 0, 1 outer, dx = 0, 1 inner, q = (ix + dx, iy + dy); bw = (dx ? wx : 1.0f - wx) * (dy ? wy : 1.0f - wy)
 *                          a tap counts iff ok, q lies in [0, width) x [row_begin, row_end), prev_guides[q].sphere == g.sphere
 *                          (MISS == MISS included), prev_colour[q].w >= 1.0f, and for a hit
 *                          fabsf(prev_guides[q].t - s) <= depth_tolerance * s;  a tap that does not count is SKIPPED
 *                          wsum += bw; acc[k] += bw * prev_colour[q][k]; lacc += bw * prev_colour[q].w      (all from +0, in tap order)
 *                  have    = wsum >= 0.015625f;  hist[k] = acc[k] / wsum;  hlen = lacc / wsum;  c[k] = colour[p][k]
 *                  with MIRT_REPROJECT_CLAMP: lo = hi = c; for dy = -1..1 outer, dx = -1..1 inner, every in-band neighbour m of p in `colour`:
 *                          lo[k] = (m[k] < lo[k]) ? m[k] : lo[k];  hi[k] = (m[k] > hi[k]) ? m[k] : hi[k]
 *                          hist[k] = (hist[k] < lo[k]) ? lo[k] : hist[k];  then hist[k] = (hist[k] > hi[k]) ? hi[k] : hist[k]
 *                  have:   nn = hlen + 1.0f; nn = (nn < max_history) ? nn : max_history; alpha = 1.0f / nn
 *                          out = {hist[k] + alpha * (c[k] - hist[k]), nn}
 *                  else:   out = {c[0], c[1], c[2], 1.0f}
 *                Every bit pattern of every input is defined by these comparisons; the previous colours may be infinite or NaN, which
 *                is why a tap that does not count is skipped and not weighted with zero.  The history is not divided by the albedo.
 *   errors       in this order.  MIRT_ERR_NULL_POINTER: any pointer but out_rgba8.  MIRT_ERR_BAD_MODE: an unknown flag, a max_history
 *                that is not finite and >= 1, a depth_tolerance that is not finite and >= 0.  MIRT_ERR_VIEWPORT_SIZE, MIRT_ERR_BAD_ROWS:
 *                as mirt_ctx_render.  MIRT_ERR_BAD_ROWS: a tile partition (n_parts > 1 with tile_rows != 0), as for the denoiser.
 *                MIRT_ERR_OUT_BUFFER: pixels < rows * width, or out / out_rgba8 overlapping any input or each other by their byte ranges
 *                (pixels records each).  A refused call queues nothing and writes nothing.
 *   state        as for every query: the launch ring, MirtStats, sums, records and sample counts are untouched;
 *                mirt_ctx_trace_stats().kernel_ms spans the kernel, mirt_ctx_last_kernel names it, mirt_ctx_synchronize and
 *                mirt_ctx_destroy wait for it.  There is no scratch: the _device form never synchronises.  The caller orders the call
 *                against those that produce its inputs (the same stream in the normal pipeline).
 *   mirt_camera_project   HOST ONLY, no device: the lines rel .. fy with rel = point - camera.eye and `camera` as `previous`; writes
 *                {fx, fy, s}: the pixel coordinates (pixel centres at integers, row 0 on top) and the ray parameter of `point`; a point
 *                is in front of the camera iff s > 0.  MIRT_ERR_NULL_POINTER for a null pointer, MIRT_ERR_VIEWPORT_SIZE for a zero size. */
typedef struct MirtReprojectParams {            /* 208 B */
    uint32_t flags;                             /* MIRT_REPROJECT_CLAMP */
    float    max_history;                       /* finite, >= 1 */
    float    depth_tolerance;                   /* finite, >= 0; relative */
    uint32_t _pad;                              /* not read */
    MirtGpuCamera previous, current;            /* the cameras the two guide frames were taken with */
} MirtReprojectParams;
typedef struct MirtReprojectFrames {            /* 56 B */
    const void* colour;
    const void* guides;
    const void* prev_colour;
    const void* prev_guides;
    void*       out;
    void*       out_rgba8;
    uint64_t    pixels;
} MirtReprojectFrames;
enum { MIRT_REPROJECT_CLAMP = 1u << 0 };
int mirt_ctx_reproject_device(MirtContext* ctx, const MirtParams* params, const MirtReprojectParams* reproject, const MirtReprojectFrames* frames, void* hip_stream);
int mirt_ctx_reproject(MirtContext* ctx, const MirtParams* params, const MirtReprojectParams* reproject, const MirtReprojectFrames* frames);   /* host memory; blocking */
int mirt_camera_project(const MirtGpuCamera* camera, uint32_t width, uint32_t height, const float point[3], float out_xy_s[3]);

/* Device self-test of the arithmetic contract: the kernels' fast sqrt and reciprocal sequences
 * (hardware seed + one fma correction) are compared with the compiler's correctly rounded IEEE
 * expansions over ALL 2^32 binary32 bit patterns.  Writes the two mismatch counts (sqrt, 1/x);
 * both must be 0 for the bit-parity claim to hold on this device. */
int mirt_ctx_selftest_math(MirtContext* ctx, uint64_t out_mismatches[2]);

/* Device self-test of the checkerboard's guarded fast path (spec S9 evaluates the sign of sin(5x) sin(5y) sin(5z) from the
 * argument reduction of the sine; the kernels first try the parity of floor(a / pi) and keep the reduction for the lanes
 * where rounding could decide).  For EVERY binary32 pattern a, as one axis: out[0] = the inputs the fast path calls decided,
 * out[1] = those among them whose parity disagrees with the reduction's sign, out[2] = those among them for which the
 * reduction reports sin(a) == 0.  out[1] and out[2] must be 0: agreement on every axis is agreement of the product, and
 * the undecided lanes run the reduction itself. */
int mirt_ctx_selftest_checker_sign(MirtContext* ctx, uint64_t out_counts[3]);

/* One-shot convenience: create context on `device`, set scene, render to host, destroy.
 * Signature a Rust `set_data` binds when it does not keep a context. */
int mirt_render(const MirtScene* scene, const MirtParams* params, int device,
                uint8_t* out_rgba8, size_t out_len);

/* RGBA8 -> RGB8 view for `Layer::imgbuf()` (layer.rs:182-186; `ImageBuffer<Rgb<u8>>`). Host-side
 * repack of n_pixels pixels. */
int mirt_rgba8_to_rgb8(const uint8_t* rgba, size_t n_pixels, uint8_t* rgb);

/* `Texture::new_from_image` (texture.rs:21-46): JPEG file bytes -> RGB8 -> `inv_255 * (p as f32)` texels, host side, so
 * that a host gets from the reference's `assets/earthmap.jpeg` / `assets/moon.jpeg` to MirtScene.texels with this
 * library alone.  Baseline and progressive Huffman JPEG, 8 bit, grey or 3 components, 4:4:4 / 4:2:2 / 4:2:0 (csrc/mirt_jpeg.cpp);
 * other files fail with MIRT_ERR_IMAGE_DECODE and a message in mirt_jpeg_last_error().  The decode is bit-identical to
 * libjpeg-turbo's (tests/test_jpeg.py); against the `image` crate it is decoder-unpinned.  No device involved. */
int mirt_jpeg_info(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height);
int mirt_jpeg_decode_rgb8(const uint8_t* data, size_t len, uint8_t* rgb, size_t rgb_len);   /* rgb_len >= width * height * 3 */
int mirt_rgb8_to_texels(const uint8_t* rgb, size_t n_pixels, float* texels);               /* texels: n_pixels x [f32;3] */
const char* mirt_jpeg_last_error(void);

/* Reassemble a full image from the `n_parts` compact buffers produced with the tile
 * interleave (root side of the multi-GPU gather).  `parts` holds n_parts buffers
 * back-to-back, each padded to `part_stride` bytes.  Device-side: both pointers are
 * device memory; runs on `hip_stream`. */
int mirt_ctx_deinterleave_device(MirtContext* ctx, const MirtParams* params, const void* d_parts,
                                 size_t part_stride, void* d_out_rgba8, size_t out_len,
                                 void* hip_stream);

/* ------------------------------------------------------------------------------------------
 * Node: ONE host process renders one frame on several devices (csrc/mirt_node.hip)
 *
 * A node drives one member context per entry of a device list.  Member i renders the rows of the 4-row tile interleave with
 * tile_rows = 4, n_parts = n, part = i; the parts are brought to member 0 and assembled there into the band image.  The result
 * is byte-identical to mirt_ctx_render of the whole band on one context, for every member count, mode and flag.
 *   transports: every entry names the SAME device -> loopback: the parts stay in the members' own buffers and the assembly
 *               reads them in place (no copies, no RCCL; exists to exercise the node on one device, no speed-up);
 *               all entries DISTINCT -> RCCL: ncclCommInitAll once in mirt_node_create, per frame one ncclGather per member
 *               (inside ncclGroupStart/End, on the member streams) of its part, padded to the largest part, into a parts
 *               buffer on member 0.  A mixed list such as {0, 1, 0} is refused.  librccl is loaded with dlopen, and only
 *               by a node that uses RCCL (an already loaded librccl first, then ROCm's): libmirt.so does not link it.
 *   params:     the node owns the partition: tile_rows, n_parts and part must be 0 (else MIRT_ERR_BAD_ROWS); every other
 *               field -- band, sample_begin, frame_spp / frame_begin, mode, flags -- reaches every member unchanged.  A member
 *               with no rows (a band of fewer than 4 * n rows) is skipped.  With n == 1 and loopback the one member renders
 *               the band straight into the output.
 *   ordering:   members render on their own context streams; the assembly waits on their render-done events (loopback)
 *               or on the gather (RCCL) with stream waits, never a host sync.  A member does not overwrite its part before
 *               the previous frame's assembly has read it (an event).  Node buffers grow and are never shrunk.
 *   errors:     MIRT_ERR_NULL_POINTER for null arguments; MIRT_ERR_NO_DEVICE for an empty list, more than
 *               MIRT_NODE_MAX_MEMBERS entries, a mixed list, MIRT_NODE_RCCL on a repeated device, a bad ordinal, or no GPU
 *               (no CPU fallback); MIRT_ERR_HIP for an RCCL failure or a missing librccl ("RCCL: ..." in mirt_last_error);
 *               MIRT_ERR_NO_SCENE for a render before a successful mirt_node_set_scene.
 *   threading:  a node is used from one host thread at a time, like a context.
 * ---------------------------------------------------------------------------------------- */
typedef struct MirtNode MirtNode;                 /* opaque */
#define MIRT_NODE_MAX_MEMBERS 16
enum {
    MIRT_NODE_RCCL = 1u << 0                      /* mirt_node_create flags: force the RCCL transport (even for n = 1) */
};
typedef struct MirtNodeStats {
    uint32_t n_members;
    uint32_t transport;                           /* 0 = same-device loopback, 1 = RCCL */
    double   gather_ms;                           /* RCCL: member 0's stream, hipEvents: all member parts ready -> gather done; 0 for loopback */
    double   assemble_ms;                         /* the assembly kernel of the last render (0 if the last render needed none) */
} MirtNodeStats;

/* Create a node of `n` members on devices[0..n).  flags: MIRT_NODE_*.  The list's shape is checked before any HIP call. */
int  mirt_node_create(const int* devices, uint32_t n, uint32_t flags, MirtNode** out);
/* Waits for everything the node queued, tears the communicators down, destroys the member contexts. */
void mirt_node_destroy(MirtNode* node);
/* mirt_ctx_set_scene on every member; if one fails the node has no scene until a later call succeeds. */
int  mirt_node_set_scene(MirtNode* node, const MirtScene* scene);
/* mirt_ctx_set_scene_ex on every member (flags: MIRT_SCENE_*; checked before any member is touched). */
int  mirt_node_set_scene_ex(MirtNode* node, const MirtScene* scene, uint32_t flags);
/* mirt_ctx_update_spheres on every member (host pointer).  If a member fails, the node has no scene until a set_scene* succeeds. */
int  mirt_node_update_spheres(MirtNode* node, uint32_t first, uint32_t count, const MirtSphere* spheres);
/* mirt_ctx_set_spheres on every member (host pointer; a device pointer belongs to one device).  The same rule on a failing member. */
int  mirt_node_set_spheres(MirtNode* node, const MirtSphere* spheres, uint32_t n_spheres);
/* mirt_ctx_set_camera on every member (host-side only). */
int  mirt_node_set_camera(MirtNode* node, const MirtGpuCamera* camera);
/* Render the band into HOST memory (mirt_params_out_rows(params) * width * 4 bytes); blocking. */
int  mirt_node_render(MirtNode* node, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);
/* Render the band into DEVICE memory on member 0's device, asynchronously: the assembly into `d_out_rgba8` is ordered after the
 * work queued so far on `hip_stream` (a hipStream_t of member 0's device; NULL = the node's own stream) and the result is ordered
 * on it.  hipStreamLegacy is refused (MIRT_ERR_HIP): pass a stream of your own. */
int  mirt_node_render_device(MirtNode* node, const MirtParams* params, void* d_out_rgba8, size_t out_len, void* hip_stream);
/* Member i's context, BORROWED (do not destroy it): per-member statistics, mirt_ctx_last_kernel, mirt_ctx_set_timing.
 * MIRT_ERR_BAD_ROWS for i >= n. */
int  mirt_node_context(MirtNode* node, uint32_t i, MirtContext** out);
/* Members and transport, and the times of the last render (waits for it). */
int  mirt_node_get_stats(MirtNode* node, MirtNodeStats* out);

/* ---- progressive accumulation on a node: the reference's render loop on several devices.  Member i owns the exact sums of ITS part
 * of the tile interleave (mirt_ctx_accum_reset with tile_rows = 4, n_parts = n, part = i); a frame runs mirt_ctx_accum_frame_device on
 * every member into its part buffer, and the parts then take the path of mirt_node_render_device: in place (loopback) or one ncclGather
 * per member, then the assembly -- same events, no host sync.  What crosses devices per frame is 4 bytes per pixel of RGBA8, never the
 * 24 bytes per pixel of sums.  Image, sums and count equal a single context's for every member count.
 *   params:  the node owns the partition (non-zero tile_rows / n_parts / part: MIRT_ERR_BAD_ROWS); a frame before a successful
 *            mirt_node_accum_reset, or with another width / height / band than the reset's: MIRT_ERR_OUT_BUFFER.  spp == 0 resolves what
 *            is there, as on a context.  A member without rows is skipped.
 *   errors:  every member is asked first, by the context's own rules, whether it would accept the frame: what a member refuses before
 *            queueing anything (MIRT_ERR_FRAME_SPP, MIRT_ERR_SPP_RANGE, MIRT_ERR_SKY, MIRT_ERR_NO_SCENE for spp == 0 on empty sums, ...)
 *            is refused up front, with the context's message, and changes nothing.  If a member's call fails after that, the node's
 *            accumulation is INVALID until the next successful mirt_node_accum_reset: frames return MIRT_ERR_OUT_BUFFER,
 *            mirt_node_accum_samples 0.
 *   mirt_node_set_scene* and mirt_node_set_camera do not touch the sums: the host resets, as with a context. ---- */
int      mirt_node_accum_reset(MirtNode* node, const MirtParams* params);
/* One progressive frame of the band into DEVICE memory on member 0's device; stream rules of mirt_node_render_device. */
int      mirt_node_accum_frame_device(MirtNode* node, const MirtParams* params, void* d_out_rgba8, size_t out_len, void* hip_stream);
/* The same frame into HOST memory; blocking. */
int      mirt_node_accum_frame(MirtNode* node, const MirtParams* params, uint8_t* out_rgba8, size_t out_len);
/* Samples per pixel accumulated since the last reset (0 for an invalid accumulation). */
uint32_t mirt_node_accum_samples(const MirtNode* node);
/* The sums of the band in band-row order, pixels x 3 uint64: the members' mirt_ctx_accum_read, every compact row placed by
 * mirt_params_out_row_index.  Blocking; meant for tests. */
int      mirt_node_accum_read(MirtNode* node, uint64_t* out_sums, size_t out_len_u64);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(MirtSphere) == 32, "Sphere is 32 B (mod.rs:418-421)");
static_assert(sizeof(MirtTextureDescriptor) == 12, "TextureDescriptor is 12 B (mod.rs:869-876)");
static_assert(sizeof(MirtMaterial) == 32, "GpuMaterial is 32 B (mod.rs:757-765)");
static_assert(sizeof(MirtGpuCamera) == 96, "GpuCamera is 96 B (mod.rs:681-697)");
static_assert(sizeof(MirtSkyState) == 144, "GpuSkyState is 144 B (mod.rs:888-896)");
static_assert(sizeof(MirtCamera) == 48, "Camera is 12 f32 (mod.rs:489-499)");
static_assert(sizeof(MirtRay) == 32, "MirtRay is two 16-byte loads");
static_assert(sizeof(MirtRayHit) == 32, "MirtRayHit is two 16-byte stores");
static_assert(sizeof(MirtRayStats) == 56, "MirtRayStats is a double and six u64");
static_assert(sizeof(MirtFeaturePixel) == 32, "MirtFeaturePixel is two 16-byte stores");
static_assert(sizeof(MirtRadianceRay) == 32, "MirtRadianceRay is two 16-byte loads");
static_assert(sizeof(MirtRadiance) == 32, "MirtRadiance is two 16-byte stores");
static_assert(sizeof(MirtRadianceParams) == 24, "MirtRadianceParams is four u32 and a u64");
static_assert(sizeof(MirtAdaptPixel) == 64, "MirtAdaptPixel is four 16-byte accesses");
static_assert(sizeof(MirtAdaptParams) == 16, "MirtAdaptParams is four u32");
static_assert(sizeof(MirtAdaptStats) == 32, "MirtAdaptStats is two u64, two u32 and a double");
static_assert(sizeof(MirtAdaptRun) == 16, "MirtAdaptRun is four u32");
static_assert(sizeof(MirtAdaptRunStep) == 8, "MirtAdaptRunStep is one 8-byte store");
static_assert(sizeof(MirtAdaptLdsPlan) == 16, "MirtAdaptLdsPlan is four words");
static_assert(sizeof(MirtDenoiseParams) == 32, "MirtDenoiseParams is eight words");
static_assert(sizeof(MirtReprojectParams) == 208, "MirtReprojectParams is four words and two cameras");
static_assert(sizeof(MirtReprojectFrames) == 56, "MirtReprojectFrames is six pointers and a count");
#else
_Static_assert(sizeof(MirtSphere) == 32, "Sphere is 32 B (mod.rs:418-421)");
_Static_assert(sizeof(MirtTextureDescriptor) == 12, "TextureDescriptor is 12 B (mod.rs:869-876)");
_Static_assert(sizeof(MirtMaterial) == 32, "GpuMaterial is 32 B (mod.rs:757-765)");
_Static_assert(sizeof(MirtGpuCamera) == 96, "GpuCamera is 96 B (mod.rs:681-697)");
_Static_assert(sizeof(MirtSkyState) == 144, "GpuSkyState is 144 B (mod.rs:888-896)");
_Static_assert(sizeof(MirtCamera) == 48, "Camera is 12 f32 (mod.rs:489-499)");
_Static_assert(sizeof(MirtRay) == 32, "MirtRay is two 16-byte loads");
_Static_assert(sizeof(MirtRayHit) == 32, "MirtRayHit is two 16-byte stores");
_Static_assert(sizeof(MirtRayStats) == 56, "MirtRayStats is a double and six u64");
_Static_assert(sizeof(MirtFeaturePixel) == 32, "MirtFeaturePixel is two 16-byte stores");
_Static_assert(sizeof(MirtRadianceRay) == 32, "MirtRadianceRay is two 16-byte loads");
_Static_assert(sizeof(MirtRadiance) == 32, "MirtRadiance is two 16-byte stores");
_Static_assert(sizeof(MirtRadianceParams) == 24, "MirtRadianceParams is four u32 and a u64");
_Static_assert(sizeof(MirtAdaptPixel) == 64, "MirtAdaptPixel is four 16-byte accesses");
_Static_assert(sizeof(MirtAdaptParams) == 16, "MirtAdaptParams is four u32");
_Static_assert(sizeof(MirtAdaptStats) == 32, "MirtAdaptStats is two u64, two u32 and a double");
_Static_assert(sizeof(MirtAdaptRun) == 16, "MirtAdaptRun is four u32");
_Static_assert(sizeof(MirtAdaptRunStep) == 8, "MirtAdaptRunStep is one 8-byte store");
_Static_assert(sizeof(MirtAdaptLdsPlan) == 16, "MirtAdaptLdsPlan is four words");
_Static_assert(sizeof(MirtDenoiseParams) == 32, "MirtDenoiseParams is eight words");
_Static_assert(sizeof(MirtReprojectParams) == 208, "MirtReprojectParams is four words and two cameras");
_Static_assert(sizeof(MirtReprojectFrames) == 56, "MirtReprojectFrames is six pointers and a count");
#endif

#endif /* MIRT_H */
