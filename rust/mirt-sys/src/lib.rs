//! Raw bindings to `include/mirt.h`.  SOURCE ONLY — never compiled in this repository (no Rust
//! toolchain in the build environment); kept in sync with the header by hand and mirrored, field
//! for field, by the ctypes binding (`weekend-raytracer-wgpu_amd/_abi.py`) whose layout IS tested.
//!
//! The wire structs are byte-identical to the reference crate's own `#[repr(C)]` types
//! (`Sphere`, `GpuMaterial`, `TextureDescriptor`, `GpuCamera`, `GpuSkyState`), so a host that
//! already has those can pass pointers to them instead of these mirrors.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtSphere {
    pub center: [f32; 4],
    pub radius: f32,
    pub material_idx: u32,
    pub _pad: [u32; 2],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtTextureDescriptor {
    pub width: u32,
    pub height: u32,
    pub offset: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtMaterial {
    pub id: u32,
    pub desc1: MirtTextureDescriptor,
    pub desc2: MirtTextureDescriptor,
    pub x: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtGpuCamera {
    pub eye: [f32; 3],
    pub _padding1: f32,
    pub horizontal: [f32; 3],
    pub _padding2: f32,
    pub vertical: [f32; 3],
    pub _padding3: f32,
    pub u: [f32; 3],
    pub _padding4: f32,
    pub v: [f32; 3],
    pub lens_radius: f32,
    pub lower_left_corner: [f32; 3],
    pub _padding5: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct MirtSkyState {
    pub params: [f32; 27],
    pub radiances: [f32; 3],
    pub _padding: [u32; 2],
    pub sun_direction: [f32; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtCamera {
    pub eye_pos: [f32; 3],
    pub eye_dir: [f32; 3],
    pub up: [f32; 3],
    pub vfov_radians: f32,
    pub aperture: f32,
    pub focus_distance: f32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtSamplingParams {
    pub max_samples_per_pixel: u32,
    pub num_samples_per_pixel: u32,
    pub num_bounces: u32,
}

#[repr(C)]
pub struct MirtScene {
    pub camera: *const MirtGpuCamera,
    pub spheres: *const MirtSphere,
    pub n_spheres: u32,
    pub materials: *const MirtMaterial,
    pub n_materials: u32,
    pub texels: *const [f32; 3],
    pub n_texels: u64,
    pub sky: *const MirtSkyState,
}

pub const MIRT_MODE_PARITY: u32 = 0;
pub const MIRT_MODE_PT: u32 = 1;
pub const MIRT_MAX_SPP_PER_CALL: u32 = 1 << 24;
pub const MIRT_FLAG_SKY_HOSEK: u32 = 1 << 0;
pub const MIRT_FLAG_NO_TONEMAP: u32 = 1 << 1;
pub const MIRT_FLAG_NO_SRGB: u32 = 1 << 2;
pub const MIRT_FLAG_COUNT_WORK: u32 = 1 << 3;
pub const MIRT_FLAG_KERNEL_STRIP: u32 = 1 << 4;
pub const MIRT_FLAG_KERNEL_POOL: u32 = 1 << 5;
pub const MIRT_FLAG_NO_GRID: u32 = 1 << 6;
pub const MIRT_FLAG_COUNT_GRID: u32 = 1 << 7;
pub const MIRT_FLAG_FAST_MATH: u32 = 1 << 8;
pub const MIRT_FLAG_TEXEL_TILES: u32 = 1 << 9;

// MirtStatus (include/mirt.h): 0 = ok, negative = error; mirt_status_string() names them, mirt_last_error() explains the last one
pub const MIRT_OK: c_int = 0;
pub const MIRT_ERR_MAX_SAMPLES_MULTIPLE: c_int = -1;
pub const MIRT_ERR_VIEWPORT_SIZE: c_int = -2;
pub const MIRT_ERR_VFOV_RANGE: c_int = -3;
pub const MIRT_ERR_APERTURE_RANGE: c_int = -4;
pub const MIRT_ERR_FOCUS_DISTANCE: c_int = -5;
pub const MIRT_ERR_SKY: c_int = -6;
pub const MIRT_ERR_NULL_POINTER: c_int = -10;
pub const MIRT_ERR_SPP_ZERO: c_int = -11;
pub const MIRT_ERR_BAD_MODE: c_int = -12;
pub const MIRT_ERR_BAD_ROWS: c_int = -13;
pub const MIRT_ERR_MATERIAL_INDEX: c_int = -14;
pub const MIRT_ERR_TEXEL_RANGE: c_int = -15;
pub const MIRT_ERR_OUT_BUFFER: c_int = -16;
pub const MIRT_ERR_NO_SCENE: c_int = -17;
pub const MIRT_ERR_SCENE_TOO_LARGE: c_int = -18;
pub const MIRT_ERR_FRAME_SPP: c_int = -19;
pub const MIRT_ERR_NO_DEVICE: c_int = -20;
pub const MIRT_ERR_HIP: c_int = -21;
pub const MIRT_ERR_ALLOC: c_int = -22;
pub const MIRT_ERR_IMAGE_DECODE: c_int = -23;
pub const MIRT_ERR_SPP_RANGE: c_int = -24;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtParams {
    pub width: u32,
    pub height: u32,
    pub spp: u32,
    pub num_bounces: u32,
    pub mode: u32,
    pub flags: u32,
    pub seed: u64,
    pub row_begin: u32,
    pub row_end: u32,
    pub tile_rows: u32,
    pub n_parts: u32,
    pub part: u32,
    pub sample_begin: u32,
    pub frame_spp: u32,
    pub frame_begin: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtGridPlan {
    pub cell_factor: f32,
    pub blob_bytes: u32,
    pub n_cells: u32,
    pub n_entries: u32,
    pub n_big: u32,
    pub pool_slots: u32,
}

/// `mirt_bvh_plan`: the BVH `mirt_ctx_set_scene_ex(.., MIRT_SCENE_HBM)` builds (host only).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtBvhPlan {
    pub n_nodes: u32,
    pub n_leaves: u32,
    pub n_leaf_spheres: u32,
    pub n_always: u32,
    pub max_depth: u32,
    pub max_leaf: u32,
    pub device_bytes: u64,
}

/// `mirt_ctx_bvh_info`: the tree a context holds (either builder), its root reference and the traversal bounds.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtBvhInfo {
    pub plan: MirtBvhPlan,
    pub root: u32,
    pub built_on_device: u32,
    pub centre: [f32; 3],
    pub radius: f32,
    pub r_max: f32,
}

/// `mirt_bvh_pool_plan`: the geometry `MIRT_FLAG_KERNEL_POOL` runs on a `MIRT_SCENE_HBM` scene (host only; `slots == 0`: none fits).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtBvhPoolPlan {
    pub threads: u32,
    pub slots: u32,
    pub waves_per_cu: u32,
    pub stack_entries: u32,
    pub lds_bytes_per_block: u32,
}

/// One ray of `mirt_ctx_trace_rays*`: `direction` is not normalised, `t_max` is the bound `closest` starts from (1000.0 = the renderer's).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRay {
    pub origin: [f32; 3],
    pub t_max: f32,
    pub direction: [f32; 3],
    pub _pad: f32,
}

/// The flat scan's answer for one ray: `sphere == MIRT_RAY_MISS` (and every other field 0) for a miss.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRayHit {
    pub t: f32,
    pub sphere: u32,
    pub point: [f32; 3],
    pub normal: [f32; 3],
}

/// `mirt_ctx_trace_stats`: of the last trace call; the counters are filled by `MIRT_RAYS_COUNT` only.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRayStats {
    pub kernel_ms: f64,
    pub rays: u64,
    pub sphere_tests: u64,
    pub roots: u64,
    pub hits: u64,
    pub nodes: u64,
    pub wave_nodes: u64,
}

/// One pixel of `mirt_ctx_render_features*`: what the camera sees first there.  `sphere == MIRT_RAY_MISS` and `t == 0` where the centre
/// ray leaves the scene; `albedo` and `normal` are means over the sample set (the centre ray alone for `spp == 0`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtFeaturePixel {
    pub albedo: [f32; 3],
    pub t: f32,
    pub normal: [f32; 3],
    pub sphere: u32,
}

/// `mirt_ctx_render_features*` flag: the flat scan instead of the tree (the comparison build).
pub const MIRT_FEATURES_FLAT: u32 = 1 << 0;

/// One ray of `mirt_ctx_trace_radiance*`.  `direction` is used as given (not normalised); `stream` selects the ray's RNG stream and
/// takes the place a pixel's index has in a render; `_pad` is not read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRadianceRay {
    pub origin: [f32; 3],
    pub stream: u32,
    pub direction: [f32; 3],
    pub _pad: u32,
}

/// One record of `mirt_ctx_trace_radiance*`: the exact sums of `samples` path-traced samples in units of 2^-20 (the mean is
/// `sum / 2^20 / samples`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRadiance {
    pub sum: [u64; 3],
    pub samples: u32,
    pub _pad: u32,
}

/// One pixel of the adaptive buffer (`mirt_ctx_adapt_*`): the exact sums of all its samples and of its even-indexed samples, 2^-20 units.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptPixel {
    pub sum: [u64; 3],
    pub even: [u64; 3],
    pub samples: u32,
    pub _pad0: u32,
    pub _pad1: u64,
}

/// The stopping rule of an adaptive step: `tolerance` is a relative error in units of 2^-16; `flags` must be 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptParams {
    pub min_samples: u32,
    pub max_samples: u32,
    pub tolerance: u32,
    pub flags: u32,
}

/// `mirt_ctx_adapt_stats`: the buffer's pixels, samples added since the reset, the last step's count, steps since the reset, its time.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptStats {
    pub pixels: u64,
    pub total_samples: u64,
    pub active: u32,
    pub steps: u32,
    pub kernel_ms: f64,
}

/// The rule's floor: 0.125 of radiance per sample, summed over the channels, in 2^-20 units.
pub const MIRT_ADAPT_FLOOR: u32 = 1 << 17;

/// An adaptive run (`mirt_ctx_adapt_run_device`): `max_steps` steps queued by one call; a step that lists `count` pixels takes
/// `spp << k` samples of each, `k` the smallest for which `count * (spp << k) >= min_items` or `spp << k == max_spp` (0: `spp`).
/// `flags` must be 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptRun {
    pub max_steps: u32,
    pub min_items: u32,
    pub max_spp: u32,
    pub flags: u32,
}

/// One entry of a run's log (`mirt_ctx_adapt_run_read`): the pixels the step listed and the samples each of them received.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptRunStep {
    pub count: u32,
    pub spp: u32,
}

/// `mirt_adapt_lds_plan`: the geometry an adaptive step with `MIRT_ADAPT_LDS` runs on a scene in LDS (host only; all fields 0: no such layout).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtAdaptLdsPlan {
    pub threads: u32,
    pub grid: u32,
    pub lds_bytes_per_block: u32,
    pub blocks_per_cu: u32,
}

/// The most steps one run queues, and the entries of its log.
pub const MIRT_ADAPT_RUN_MAX_STEPS: u32 = 256;

/// What a `mirt_ctx_trace_radiance*` call traces: samples `sample_begin .. sample_begin + spp - 1` of every ray's stream.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtRadianceParams {
    pub spp: u32,
    pub sample_begin: u32,
    pub num_bounces: u32,
    pub flags: u32,
    pub seed: u64,
}

/// `MirtRadianceParams.flags`: the flat scan instead of the tree; add to the records instead of overwriting them; the scene's Hosek sky.
pub const MIRT_RADIANCE_FLAT: u32 = 1 << 0;
pub const MIRT_RADIANCE_ACCUMULATE: u32 = 1 << 1;
pub const MIRT_RADIANCE_SKY_HOSEK: u32 = 1 << 2;
/// The batch runs in an order the library derives on the device; same records.  Bit 3 is unassigned.
pub const MIRT_RADIANCE_SORT: u32 = 1 << 4;
/// A hint: the pooled schedule (a wave deals the samples of 16 rays to its lanes); same records.  Bit 5 is unassigned.
pub const MIRT_RADIANCE_POOL: u32 = 1 << 6;
/// `MirtAdaptParams.flags`: the pooled schedule for the step's render stage (a hint: same records); bit 0 is unassigned.
pub const MIRT_ADAPT_POOL: u32 = 1 << 1;
/// `MirtAdaptParams.flags`: a step or run also accepts a scene that lives in LDS, where it stays (an HBM scene ignores it); bit 2 is unassigned.
pub const MIRT_ADAPT_LDS: u32 = 1 << 3;
/// The parameters of `mirt_ctx_denoise*`: the edge-avoiding a-trous filter over the accumulation or the adaptive records.  `_pad` is not read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct MirtDenoiseParams {
    pub source: u32,
    pub levels: u32,
    pub normal_log2: u32,
    pub flags: u32,
    pub sigma_colour: f32,
    pub _pad: [u32; 3],
}
/// `MirtDenoiseParams.source`: the context's accumulation buffer, or its adaptive records.
pub const MIRT_DENOISE_SRC_ACCUM: u32 = 0;
pub const MIRT_DENOISE_SRC_ADAPT: u32 = 1;
/// `MirtDenoiseParams.flags`: the output is `{r, g, b, 1.0}` as float32 (the linear mean), not RGBA8.
pub const MIRT_DENOISE_OUT_F32: u32 = 1 << 0;
/// The parameters of `mirt_ctx_reproject*`: temporal reprojection by first-hit depth and id.  `previous` and `current` are the cameras the
/// two guide frames were taken with; `_pad` is not read.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtReprojectParams {
    pub flags: u32,
    pub max_history: f32,
    pub depth_tolerance: f32,
    pub _pad: u32,
    pub previous: MirtGpuCamera,
    pub current: MirtGpuCamera,
}
/// The planes of `mirt_ctx_reproject*`: all device pointers (the `_device` form) or all host pointers, 4-byte aligned, `pixels` records
/// each; `out_rgba8` may be null.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct MirtReprojectFrames {
    pub colour: *const c_void,
    pub guides: *const c_void,
    pub prev_colour: *const c_void,
    pub prev_guides: *const c_void,
    pub out: *mut c_void,
    pub out_rgba8: *mut c_void,
    pub pixels: u64,
}
/// `MirtReprojectParams.flags`: the history is clamped to the colours of the pixel's 3 x 3 neighbourhood in this frame.
pub const MIRT_REPROJECT_CLAMP: u32 = 1 << 0;

/// The `flags` of `mirt_ctx_trace_rays*` and `mirt_ctx_render_features*`, and `MirtRadianceParams.flags`: the query also accepts a scene
/// that lives in LDS, where it stays (the same records as on the same world held as an HBM scene, which ignores the flag).
pub const MIRT_QUERY_LDS: u32 = 1 << 8;

pub const MIRT_RAY_MISS: u32 = 0xffff_ffff;
/// `mirt_ctx_trace_rays*` flags: the flat scan instead of the tree; stop at the first hit (occlusion); the counting build.
pub const MIRT_RAYS_FLAT: u32 = 1 << 0;
pub const MIRT_RAYS_ANY_HIT: u32 = 1 << 1;
pub const MIRT_RAYS_COUNT: u32 = 1 << 2;
/// The batch is traced in an order the library derives on the device; same hits.  Bit 3 is unassigned.
pub const MIRT_RAYS_SORT: u32 = 1 << 4;
/// Bits per origin axis / per octahedral direction axis of `mirt_ray_sort_code`.
pub const MIRT_RAY_SORT_ORIGIN_BITS: u32 = 5;
pub const MIRT_RAY_SORT_DIRECTION_BITS: u32 = 8;

/// `mirt_ctx_set_scene_ex` / `mirt_node_set_scene_ex` flags: the scene's tables in device memory, nearest hit through a BVH
/// (worlds beyond the LDS budget, up to `MIRT_SCENE_HBM_MAX_SPHERES`).
pub const MIRT_SCENE_HBM: u32 = 1 << 0;
/// Only together with `MIRT_SCENE_HBM`: build the BVH on the device.
pub const MIRT_SCENE_BVH_DEVICE: u32 = 1 << 1;
pub const MIRT_SCENE_HBM_MAX_SPHERES: u32 = 1 << 24;
pub const MIRT_BVH_MAX_DEPTH: u32 = 32;
pub const MIRT_BVH_MAX_LEAF: u32 = 4;
pub const MIRT_BVH_MAX_ALWAYS: u32 = 64;
pub const MIRT_BVH_BIG_RADII: u32 = 4;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtStats {
    pub kernel_ms: f64,
    pub kernel_ms_total: f64,
    pub launches: u64,
    pub samples: u64,
    pub rays: u64,
    pub sphere_tests: u64,
    pub roots: u64,
    pub hits: u64,
    pub scatter: [u64; 5],
    pub sky_misses: u64,
    pub lane_iterations: u64,
    pub wave_iterations: u64,
    pub grid_cells: u64,
    pub grid_wave_cells: u64,
    pub texel_fetches: [u64; 2],
    pub texel_tile_hits: [u64; 2],
}

#[repr(C)]
pub struct MirtContext {
    _private: [u8; 0],
}

// Node: one process renders one frame on several devices (mirt_node_*, include/mirt.h)
pub const MIRT_NODE_MAX_MEMBERS: u32 = 16;
pub const MIRT_NODE_RCCL: u32 = 1 << 0;

#[repr(C)]
pub struct MirtNode {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct MirtNodeStats {
    pub n_members: u32,
    pub transport: u32,
    pub gather_ms: f64,
    pub assemble_ms: f64,
}

extern "C" {
    pub fn mirt_version() -> u32;
    pub fn mirt_last_error() -> *const c_char;
    pub fn mirt_status_string(status: c_int) -> *const c_char;
    pub fn mirt_validate_render_params(camera: *const MirtCamera, sampling: *const MirtSamplingParams, viewport_w: u32, viewport_h: u32) -> c_int;
    pub fn mirt_camera_new(camera: *const MirtCamera, viewport_w: u32, viewport_h: u32, out: *mut MirtGpuCamera) -> c_int;
    pub fn mirt_camera_from_fly_pose(position: *const f32, yaw_radians: f32, pitch_radians: f32, vfov_degrees: f32, aperture: f32, focus_distance: f32, out: *mut MirtCamera) -> c_int;
    pub fn mirt_degrees_to_radians(degrees: f32) -> f32;
    pub fn mirt_radians_to_degrees(radians: f32) -> f32;
    pub fn mirt_params_out_rows(params: *const MirtParams) -> u32;
    pub fn mirt_params_out_row_index(params: *const MirtParams, i: u32) -> u32;
    pub fn mirt_grid_plan(spheres: *const MirtSphere, n_spheres: u32, lds_bytes_per_block: u64, out: *mut MirtGridPlan) -> c_int;
    pub fn mirt_ctx_create(device: c_int, out: *mut *mut MirtContext) -> c_int;
    pub fn mirt_ctx_destroy(ctx: *mut MirtContext);
    pub fn mirt_ctx_set_scene(ctx: *mut MirtContext, scene: *const MirtScene) -> c_int;
    pub fn mirt_ctx_set_scene_ex(ctx: *mut MirtContext, scene: *const MirtScene, flags: u32) -> c_int;
    pub fn mirt_bvh_plan(spheres: *const MirtSphere, n_spheres: u32, out: *mut MirtBvhPlan) -> c_int;
    pub fn mirt_bvh_pool_plan(max_depth: u32, hosek: u32, lds_bytes_per_cu: u64, out: *mut MirtBvhPoolPlan) -> c_int;
    pub fn mirt_adapt_pool_plan(max_depth: u32, hosek: u32, lds_bytes_per_cu: u64, out: *mut MirtBvhPoolPlan) -> c_int;
    pub fn mirt_ctx_bvh_info(ctx: *mut MirtContext, out: *mut MirtBvhInfo) -> c_int;
    pub fn mirt_ctx_bvh_read(ctx: *mut MirtContext, nodes: *mut c_void, nodes_bytes: usize, recs: *mut f32, recs_len: usize, ids: *mut u32, ids_len: usize) -> c_int;
    pub fn mirt_ctx_update_spheres(ctx: *mut MirtContext, first: u32, count: u32, spheres: *const MirtSphere) -> c_int;
    pub fn mirt_ctx_update_spheres_device(ctx: *mut MirtContext, first: u32, count: u32, d_spheres: *const c_void) -> c_int;
    pub fn mirt_ctx_bvh_refits(ctx: *const MirtContext) -> u32;
    pub fn mirt_ctx_set_spheres(ctx: *mut MirtContext, spheres: *const MirtSphere, n_spheres: u32) -> c_int;
    pub fn mirt_ctx_set_spheres_device(ctx: *mut MirtContext, d_spheres: *const c_void, n_spheres: u32) -> c_int;
    pub fn mirt_ctx_trace_rays(ctx: *mut MirtContext, rays: *const MirtRay, n_rays: u32, flags: u32, hits: *mut MirtRayHit) -> c_int;
    pub fn mirt_ctx_trace_rays_device(ctx: *mut MirtContext, d_rays: *const c_void, n_rays: u32, flags: u32, d_hits: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_trace_stats(ctx: *mut MirtContext, out: *mut MirtRayStats) -> c_int;
    pub fn mirt_ctx_render_features(ctx: *mut MirtContext, params: *const MirtParams, flags: u32, out: *mut MirtFeaturePixel, out_len: usize) -> c_int;
    pub fn mirt_ctx_render_features_device(ctx: *mut MirtContext, params: *const MirtParams, flags: u32, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_camera_pixel_ray(camera: *const MirtGpuCamera, width: u32, height: u32, x: u32, y: u32, out: *mut MirtRay) -> c_int;
    pub fn mirt_ctx_trace_radiance(ctx: *mut MirtContext, rays: *const MirtRadianceRay, n_rays: u32, params: *const MirtRadianceParams, out: *mut MirtRadiance) -> c_int;
    pub fn mirt_ctx_trace_radiance_device(ctx: *mut MirtContext, d_rays: *const c_void, n_rays: u32, params: *const MirtRadianceParams, d_out: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ray_sort_code(centre: *const f32, radius: f32, ray32: *const c_void, out_code: *mut u32) -> c_int;
    pub fn mirt_ctx_trace_order_read(ctx: *mut MirtContext, order: *mut u32, len: usize) -> c_int;
    pub fn mirt_ctx_set_camera(ctx: *mut MirtContext, camera: *const MirtGpuCamera) -> c_int;
    pub fn mirt_ctx_render(ctx: *mut MirtContext, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_ctx_render_device(ctx: *mut MirtContext, params: *const MirtParams, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_synchronize(ctx: *mut MirtContext) -> c_int;
    pub fn mirt_ctx_get_stats(ctx: *mut MirtContext, out: *mut MirtStats) -> c_int;
    pub fn mirt_ctx_frame_stream(ctx: *mut MirtContext, index: u32, out_hip_stream: *mut *mut c_void) -> c_int;
    pub fn mirt_ctx_set_timing(ctx: *mut MirtContext, enabled: c_int) -> c_int;
    pub fn mirt_ctx_last_kernel(ctx: *const MirtContext) -> *const c_char;
    pub fn mirt_ctx_accum_reset(ctx: *mut MirtContext, params: *const MirtParams) -> c_int;
    pub fn mirt_ctx_accum_add(ctx: *mut MirtContext, params: *const MirtParams, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_accum_samples(ctx: *const MirtContext) -> u32;
    pub fn mirt_ctx_accum_resolve(ctx: *mut MirtContext, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_ctx_accum_read(ctx: *mut MirtContext, out_sums: *mut u64, out_len_u64: usize) -> c_int;
    pub fn mirt_ctx_accum_frame_device(ctx: *mut MirtContext, params: *const MirtParams, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_accum_frame(ctx: *mut MirtContext, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    // adaptive sampling for progressive frames of a MIRT_SCENE_HBM scene (include/mirt.h: mirt_ctx_adapt_*)
    pub fn mirt_adapt_active(pixel: *const MirtAdaptPixel, adapt: *const MirtAdaptParams, out: *mut u32) -> c_int;
    pub fn mirt_ctx_adapt_reset(ctx: *mut MirtContext, params: *const MirtParams) -> c_int;
    pub fn mirt_ctx_adapt_step_device(ctx: *mut MirtContext, params: *const MirtParams, adapt: *const MirtAdaptParams, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_adapt_resolve_device(ctx: *mut MirtContext, params: *const MirtParams, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_adapt_resolve(ctx: *mut MirtContext, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_ctx_adapt_read(ctx: *mut MirtContext, out: *mut MirtAdaptPixel, len: usize) -> c_int;
    pub fn mirt_ctx_adapt_write(ctx: *mut MirtContext, input: *const MirtAdaptPixel, len: usize) -> c_int;
    pub fn mirt_ctx_adapt_list_read(ctx: *mut MirtContext, list: *mut u32, len: usize, count: *mut u32) -> c_int;
    pub fn mirt_ctx_adapt_stats(ctx: *mut MirtContext, out: *mut MirtAdaptStats) -> c_int;
    // adaptive runs: a whole loop per call, step sizes chosen on the device
    pub fn mirt_adapt_run_spp(count: u32, spp: u32, run: *const MirtAdaptRun, out: *mut u32) -> c_int;
    pub fn mirt_ctx_adapt_run_device(ctx: *mut MirtContext, params: *const MirtParams, adapt: *const MirtAdaptParams, run: *const MirtAdaptRun, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_adapt_run_read(ctx: *mut MirtContext, out: *mut MirtAdaptRunStep, len: usize, n_steps: *mut u32) -> c_int;
    // adaptive steps on a scene that lives in LDS (MIRT_ADAPT_LDS): the launch's geometry and the device's rule for the sample groups, host only
    pub fn mirt_ctx_denoise_device(ctx: *mut MirtContext, params: *const MirtParams, denoise: *const MirtDenoiseParams, d_guides: *const c_void, guides_len: usize, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_denoise(ctx: *mut MirtContext, params: *const MirtParams, denoise: *const MirtDenoiseParams, guides: *const MirtFeaturePixel, guides_len: usize, out: *mut c_void, out_len: usize) -> c_int;
    pub fn mirt_ctx_reproject_device(ctx: *mut MirtContext, params: *const MirtParams, reproject: *const MirtReprojectParams, frames: *const MirtReprojectFrames, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_ctx_reproject(ctx: *mut MirtContext, params: *const MirtParams, reproject: *const MirtReprojectParams, frames: *const MirtReprojectFrames) -> c_int;
    pub fn mirt_camera_project(camera: *const MirtGpuCamera, width: u32, height: u32, point: *const f32, out_xy_s: *mut f32) -> c_int;
    pub fn mirt_adapt_lds_plan(n_spheres: u32, n_materials: u32, grid_bytes: u32, hosek: u32, lds_bytes_per_cu: u64, out: *mut MirtAdaptLdsPlan) -> c_int;
    pub fn mirt_adapt_lds_groups(count: u32, spp: u32, grid_waves: u32, out_log2: *mut u32) -> c_int;
    pub fn mirt_ctx_selftest_math(ctx: *mut MirtContext, out_mismatches: *mut u64) -> c_int;
    pub fn mirt_ctx_selftest_checker_sign(ctx: *mut MirtContext, out_counts: *mut u64) -> c_int;
    pub fn mirt_render(scene: *const MirtScene, params: *const MirtParams, device: c_int, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_rgba8_to_rgb8(rgba: *const u8, n_pixels: usize, rgb: *mut u8) -> c_int;
    // `Texture::new_from_image` (texture.rs:21-46) without the `image` crate: JPEG bytes -> RGB8 -> [f32;3] texels
    pub fn mirt_jpeg_info(data: *const u8, len: usize, width: *mut u32, height: *mut u32) -> c_int;
    pub fn mirt_jpeg_decode_rgb8(data: *const u8, len: usize, rgb: *mut u8, rgb_len: usize) -> c_int;
    pub fn mirt_rgb8_to_texels(rgb: *const u8, n_pixels: usize, texels: *mut f32) -> c_int;
    pub fn mirt_jpeg_last_error() -> *const c_char;
    pub fn mirt_ctx_deinterleave_device(ctx: *mut MirtContext, params: *const MirtParams, d_parts: *const c_void, part_stride: usize, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_node_create(devices: *const c_int, n: u32, flags: u32, out: *mut *mut MirtNode) -> c_int;
    pub fn mirt_node_destroy(node: *mut MirtNode);
    pub fn mirt_node_set_scene(node: *mut MirtNode, scene: *const MirtScene) -> c_int;
    pub fn mirt_node_set_scene_ex(node: *mut MirtNode, scene: *const MirtScene, flags: u32) -> c_int;
    pub fn mirt_node_update_spheres(node: *mut MirtNode, first: u32, count: u32, spheres: *const MirtSphere) -> c_int;
    pub fn mirt_node_set_spheres(node: *mut MirtNode, spheres: *const MirtSphere, n_spheres: u32) -> c_int;
    pub fn mirt_node_set_camera(node: *mut MirtNode, camera: *const MirtGpuCamera) -> c_int;
    pub fn mirt_node_render(node: *mut MirtNode, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_node_render_device(node: *mut MirtNode, params: *const MirtParams, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_node_context(node: *mut MirtNode, i: u32, out: *mut *mut MirtContext) -> c_int;
    pub fn mirt_node_get_stats(node: *mut MirtNode, out: *mut MirtNodeStats) -> c_int;
    pub fn mirt_node_accum_reset(node: *mut MirtNode, params: *const MirtParams) -> c_int;
    pub fn mirt_node_accum_frame_device(node: *mut MirtNode, params: *const MirtParams, d_out_rgba8: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn mirt_node_accum_frame(node: *mut MirtNode, params: *const MirtParams, out_rgba8: *mut u8, out_len: usize) -> c_int;
    pub fn mirt_node_accum_samples(node: *const MirtNode) -> u32;
    pub fn mirt_node_accum_read(node: *mut MirtNode, out_sums: *mut u64, out_len_u64: usize) -> c_int;
}
