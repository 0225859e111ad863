// mirt_host.hpp — C++ mirror of the reference's Rust interface for the per-pixel path
// (src/raytracer/{mod,layer,texture,angle}.rs, src/fly_camera.rs), sitting directly on the C ABI
// of include/mirt.h.  Same names, argument meaning and error behaviour; `Layer::set_data` is ONE
// FFI call.  Header-only; link with -lmirt.  No pixel is computed on the host.
#pragma once

#include <array>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include "../../include/mirt.h"

namespace mirt_host {

struct Vec3 { float x, y, z; };

// RenderParamsValidationError (mod.rs:396-411) and every other negative status
struct MirtError : std::runtime_error {
    int status;
    MirtError(int s, const std::string& what) : std::runtime_error(std::string(mirt_status_string(s)) + ": " + what), status(s) {}
};
inline void check(int rc) { if (rc != MIRT_OK) throw MirtError(rc, mirt_last_error()); }

// mirt_ctx_set_scene, and a world the LDS layouts refuse (MIRT_ERR_SCENE_TOO_LARGE) set again with MIRT_SCENE_HBM: the reference's
// `Layer::set_data` takes any `Vec<Box<Sphere>>`
// (*hbm, when given: whether the scene went to device memory -- its spheres can then be moved in place, update_spheres below)
inline int set_scene_any_size(MirtContext* ctx, const MirtScene& sc, bool* hbm = nullptr)
{
    const int rc = mirt_ctx_set_scene(ctx, &sc);
    if (hbm) *hbm = rc == MIRT_ERR_SCENE_TOO_LARGE;
    return rc == MIRT_ERR_SCENE_TOO_LARGE ? mirt_ctx_set_scene_ex(ctx, &sc, MIRT_SCENE_HBM) : rc;
}
// mirt_ctx_set_scene_ex: flags = MIRT_SCENE_*
inline void set_scene(MirtContext* ctx, const MirtScene& sc, uint32_t flags) { check(mirt_ctx_set_scene_ex(ctx, &sc, flags)); }
// mirt_ctx_bvh_info: the tree of the context's MIRT_SCENE_HBM scene (built on the host, or on the device with MIRT_SCENE_BVH_DEVICE)
inline MirtBvhInfo bvh_info(MirtContext* ctx) { MirtBvhInfo info; check(mirt_ctx_bvh_info(ctx, &info)); return info; }
// mirt_bvh_pool_plan: the geometry MIRT_FLAG_KERNEL_POOL runs on a MIRT_SCENE_HBM scene whose tree is `max_depth` deep (host only;
// slots == 0: none fits, the launch runs the strip kernel)
inline MirtBvhPoolPlan bvh_pool_plan(uint32_t max_depth, bool hosek = false, uint64_t lds_bytes_per_cu = 0)
{
    MirtBvhPoolPlan plan;
    check(mirt_bvh_pool_plan(max_depth, hosek ? 1u : 0u, lds_bytes_per_cu, &plan));
    return plan;
}
// mirt_ctx_update_spheres: spheres first .. first + count of a MIRT_SCENE_HBM scene take centre and radius from `spheres` (material_idx
// is not read); the BVH is refitted on the device.  mirt_ctx_bvh_refits counts the updates since the scene was set.
inline void update_spheres(MirtContext* ctx, uint32_t first, const std::vector<MirtSphere>& spheres)
{
    check(mirt_ctx_update_spheres(ctx, first, (uint32_t)spheres.size(), spheres.data()));
}
// the same from records in memory of the context's device
inline void update_spheres_device(MirtContext* ctx, uint32_t first, uint32_t count, const void* d_spheres)
{
    check(mirt_ctx_update_spheres_device(ctx, first, count, d_spheres));
}
inline uint32_t bvh_refits(const MirtContext* ctx) { return mirt_ctx_bvh_refits(ctx); }
// mirt_ctx_set_spheres: a MIRT_SCENE_HBM scene gets `spheres` as its new sphere table (any count; material_idx is read) and a tree built
// on the device; camera, materials, texels and sky stay resident.
inline void set_spheres(MirtContext* ctx, const std::vector<MirtSphere>& spheres)
{
    check(mirt_ctx_set_spheres(ctx, spheres.data(), (uint32_t)spheres.size()));
}
// the same from records in memory of the context's device
inline void set_spheres_device(MirtContext* ctx, const void* d_spheres, uint32_t n_spheres)
{
    check(mirt_ctx_set_spheres_device(ctx, d_spheres, n_spheres));
}
// mirt_ctx_trace_rays: the flat scan's answer for every ray against the context's MIRT_SCENE_HBM scene, in the caller's order
// (flags = MIRT_RAYS_*; hit.sphere == MIRT_RAY_MISS: nothing hit).  Blocking.
inline MirtRay make_ray(Vec3 origin, Vec3 direction, float t_max = 1000.0f)
{
    return MirtRay{ { origin.x, origin.y, origin.z }, t_max, { direction.x, direction.y, direction.z }, 0.0f };
}
inline std::vector<MirtRayHit> trace_rays(MirtContext* ctx, const std::vector<MirtRay>& rays, uint32_t flags = 0)
{
    std::vector<MirtRayHit> hits(rays.size());
    check(mirt_ctx_trace_rays(ctx, rays.data(), (uint32_t)rays.size(), flags, hits.data()));
    return hits;
}
// the same between buffers in memory of the context's device, asynchronously on `hip_stream` (nullptr: the context's stream)
inline void trace_rays_device(MirtContext* ctx, const void* d_rays, uint32_t n_rays, void* d_hits, uint32_t flags = 0, void* hip_stream = nullptr)
{
    check(mirt_ctx_trace_rays_device(ctx, d_rays, n_rays, flags, d_hits, hip_stream));
}
inline MirtRayStats trace_stats(MirtContext* ctx) { MirtRayStats st; check(mirt_ctx_trace_stats(ctx, &st)); return st; }
// mirt_ctx_render_features: what the context's camera sees first at every pixel of the rows `params` selects -- albedo, depth, normal
// and sphere id, compact and row-major like a render; params.spp == 0 traces the centre rays alone, flags = MIRT_FEATURES_*.  Blocking.
inline std::vector<MirtFeaturePixel> render_features(MirtContext* ctx, const MirtParams& params, uint32_t flags = 0)
{
    std::vector<MirtFeaturePixel> out((size_t)mirt_params_out_rows(&params) * params.width);
    MirtFeaturePixel none{};
    check(mirt_ctx_render_features(ctx, &params, flags, out.empty() ? &none : out.data(), out.size() * sizeof(MirtFeaturePixel)));
    return out;
}
// mirt_ctx_denoise: the edge-avoiding a-trous filter over the context's accumulation (denoise.source = MIRT_DENOISE_SRC_ACCUM) or its
// adaptive records (MIRT_DENOISE_SRC_ADAPT), guided by `guides` -- what render_features returned for the same params' width, height and
// rows -> the band's bytes: RGBA8, or {r, g, b, 1.0f} as float32 with MIRT_DENOISE_OUT_F32.  Reads no scene; blocking.
static_assert(sizeof(MirtDenoiseParams) == 32 && MIRT_DENOISE_SRC_ADAPT == 1 && MIRT_DENOISE_OUT_F32 == 1u << 0, "MirtDenoiseParams");
inline MirtDenoiseParams denoise_params(uint32_t source = MIRT_DENOISE_SRC_ACCUM, uint32_t levels = 3, float sigma_colour = 1.0f, uint32_t normal_log2 = 5, bool f32 = false)
{
    MirtDenoiseParams d{};
    d.source = source; d.levels = levels; d.normal_log2 = normal_log2; d.flags = f32 ? (uint32_t)MIRT_DENOISE_OUT_F32 : 0u; d.sigma_colour = sigma_colour;
    return d;
}
inline std::vector<uint8_t> denoise(MirtContext* ctx, const MirtParams& params, const MirtDenoiseParams& denoise, const std::vector<MirtFeaturePixel>& guides)
{
    const size_t px = (denoise.flags & MIRT_DENOISE_OUT_F32) ? 16u : 4u;
    std::vector<uint8_t> out((size_t)mirt_params_out_rows(&params) * params.width * px);
    uint8_t none[16] = {};
    MirtFeaturePixel no_guide{};
    check(mirt_ctx_denoise(ctx, &params, &denoise, guides.empty() ? &no_guide : guides.data(), guides.size() * sizeof(MirtFeaturePixel),
                           out.empty() ? none : out.data(), out.size()));
    return out;
}
inline void denoise_device(MirtContext* ctx, const MirtParams& params, const MirtDenoiseParams& denoise, const void* d_guides, size_t guides_len, void* d_out,
                           size_t out_len, void* hip_stream = nullptr)
{
    check(mirt_ctx_denoise_device(ctx, &params, &denoise, d_guides, guides_len, d_out, out_len, hip_stream));
}
// mirt_ctx_reproject: this frame's `colour` ({r, g, b, ignored} as float32, what denoise wrote with MIRT_DENOISE_OUT_F32) blended with the
// previous frame's result `prev_colour` ({r, g, b, history length}) taken to this frame's pixels by the first-hit depth and id of the two
// guide frames -> {r, g, b, new history length} per pixel of the band; `rgba8` non-null: also the RGBA8 pixels per params.flags.  Reads no
// scene; blocking.
static_assert(sizeof(MirtReprojectParams) == 208 && sizeof(MirtReprojectFrames) == 56 && MIRT_REPROJECT_CLAMP == 1u << 0, "MirtReprojectParams");
inline MirtReprojectParams reproject_params(const MirtGpuCamera& previous, const MirtGpuCamera& current, float max_history = 4.0f, float depth_tolerance = 0.05f,
                                            bool clamp = true)
{
    MirtReprojectParams r{};
    r.flags = clamp ? (uint32_t)MIRT_REPROJECT_CLAMP : 0u; r.max_history = max_history; r.depth_tolerance = depth_tolerance;
    r.previous = previous; r.current = current;
    return r;
}
inline std::vector<float> reproject(MirtContext* ctx, const MirtParams& params, const MirtReprojectParams& reproject, const std::vector<float>& colour,
                                    const std::vector<MirtFeaturePixel>& guides, const std::vector<float>& prev_colour,
                                    const std::vector<MirtFeaturePixel>& prev_guides, std::vector<uint8_t>* rgba8 = nullptr)
{
    const size_t n = (size_t)mirt_params_out_rows(&params) * params.width;
    if (colour.size() < 4u * n || prev_colour.size() < 4u * n || guides.size() < n || prev_guides.size() < n)
        throw std::invalid_argument("mirt_host::reproject: a plane holds fewer records than the band has pixels");
    std::vector<float> out(4u * n);
    if (rgba8) rgba8->assign(4u * n, 0u);
    float none[4] = {};
    uint8_t no_px[4] = {};
    MirtFeaturePixel no_guide{};
    MirtReprojectFrames f{};
    f.colour = n ? (const void*)colour.data() : none; f.prev_colour = n ? (const void*)prev_colour.data() : none;
    f.guides = n ? guides.data() : &no_guide; f.prev_guides = n ? prev_guides.data() : &no_guide;
    f.out = n ? out.data() : none;
    f.out_rgba8 = rgba8 ? (n ? rgba8->data() : no_px) : nullptr;
    f.pixels = n;
    check(mirt_ctx_reproject(ctx, &params, &reproject, &f));
    return out;
}
inline void reproject_device(MirtContext* ctx, const MirtParams& params, const MirtReprojectParams& reproject, const MirtReprojectFrames& d_frames,
                             void* hip_stream = nullptr)
{
    check(mirt_ctx_reproject_device(ctx, &params, &reproject, &d_frames, hip_stream));
}
// where `point` falls in the viewport: {fx, fy, s} (mirt_camera_project: pixel centres at integers, row 0 on top; s > 0 in front of the camera)
inline std::array<float, 3> camera_project(const MirtGpuCamera& cam, uint32_t width, uint32_t height, const std::array<float, 3>& point)
{
    std::array<float, 3> out{};
    check(mirt_camera_project(&cam, width, height, point.data(), out.data()));
    return out;
}
// the centre ray of pixel (x, y) exactly as the feature kernel traces it (mirt_camera_pixel_ray: float32 with fmaf, t_max = 1000)
inline MirtRay camera_pixel_ray(const MirtGpuCamera& cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y)
{
    MirtRay r{};
    check(mirt_camera_pixel_ray(&cam, width, height, x, y, &r));
    return r;
}
// mirt_ctx_trace_radiance: params.spp samples of the path tracer for every ray (the renderer's samples from the primary ray on; `stream`
// of a ray takes the place of a pixel's index) -> one record of exact sums per ray; params.flags = MIRT_RADIANCE_* (the records start at zero, so _ACCUMULATE changes nothing here);
// MIRT_RADIANCE_POOL among them asks for the pooled schedule (a hint: same records).  Blocking.
static_assert(MIRT_RADIANCE_POOL == 1u << 6, "MirtRadianceParams.flags: the pooled schedule");
inline std::vector<MirtRadiance> trace_radiance(MirtContext* ctx, const std::vector<MirtRadianceRay>& rays, const MirtRadianceParams& params)
{
    std::vector<MirtRadiance> out(rays.size());
    check(mirt_ctx_trace_radiance(ctx, rays.data(), (uint32_t)rays.size(), &params, out.data()));
    return out;
}
// mirt_ray_sort_code: the 31-bit code MIRT_RAYS_SORT / MIRT_RADIANCE_SORT order a batch by, for one 32-byte record (MirtRay or
// MirtRadianceRay); centre, radius: those of mirt_ctx_bvh_info.  Host only.
inline uint32_t ray_sort_code(const float centre[3], float radius, const void* ray32)
{
    uint32_t code = 0;
    check(mirt_ray_sort_code(centre, radius, ray32, &code));
    return code;
}
// mirt_ctx_trace_order_read: the permutation of the last sorted launch of `n_rays` rays; order[k] = the caller's index of the ray in slot k
inline std::vector<uint32_t> trace_order(MirtContext* ctx, uint32_t n_rays)
{
    std::vector<uint32_t> order(n_rays ? n_rays : 1u);
    check(mirt_ctx_trace_order_read(ctx, order.data(), order.size()));
    order.resize(n_rays);
    return order;
}
// mirt_ctx_adapt_* (adaptive sampling for progressive frames of a MIRT_SCENE_HBM scene): thin wrappers.  adapt_reset sizes and clears the
// records for the rows `params` selects; adapt_step queues one step (select, then params.spp -- even -- further samples for every active pixel)
// on `hip_stream` and returns at once; the others block.  adapt_active is the rule for one record, host only.
static_assert(sizeof(MirtAdaptPixel) == 64 && sizeof(MirtAdaptParams) == 16 && MIRT_ADAPT_FLOOR == 1u << 17, "the adaptive records of include/mirt.h");
inline bool adapt_active(const MirtAdaptPixel& pixel, const MirtAdaptParams& adapt)
{
    uint32_t on = 0;
    check(mirt_adapt_active(&pixel, &adapt, &on));
    return on != 0u;
}
// MIRT_ADAPT_POOL in MirtAdaptParams.flags asks for the pooled schedule of the step's render stage (a hint: same records).
static_assert(MIRT_ADAPT_POOL == 1u << 1, "MirtAdaptParams.flags: the pooled schedule");
// mirt_adapt_pool_plan: the geometry such a step runs on a tree `max_depth` deep (host only; slots == 0: none fits, the step runs as without the flag)
inline MirtBvhPoolPlan adapt_pool_plan(uint32_t max_depth, bool hosek = false, uint64_t lds_bytes_per_cu = 0)
{
    MirtBvhPoolPlan plan;
    check(mirt_adapt_pool_plan(max_depth, hosek ? 1u : 0u, lds_bytes_per_cu, &plan));
    return plan;
}
inline void adapt_reset(MirtContext* ctx, const MirtParams& params) { check(mirt_ctx_adapt_reset(ctx, &params)); }
inline void adapt_step(MirtContext* ctx, const MirtParams& params, const MirtAdaptParams& adapt, void* hip_stream = nullptr)
{
    check(mirt_ctx_adapt_step_device(ctx, &params, &adapt, hip_stream));
}
inline MirtAdaptStats adapt_stats(MirtContext* ctx)
{
    MirtAdaptStats st{};
    check(mirt_ctx_adapt_stats(ctx, &st));
    return st;
}
inline std::vector<uint8_t> adapt_resolve(MirtContext* ctx, const MirtParams& params)
{
    std::vector<uint8_t> out((size_t)adapt_stats(ctx).pixels * 4u);
    uint8_t none[4];
    check(mirt_ctx_adapt_resolve(ctx, &params, out.empty() ? none : out.data(), out.size()));
    return out;
}
// the same resolve into `out_len` bytes of device memory on `hip_stream`, no host synchronisation
inline void adapt_resolve_device(MirtContext* ctx, const MirtParams& params, void* d_out_rgba8, size_t out_len, void* hip_stream = nullptr)
{
    check(mirt_ctx_adapt_resolve_device(ctx, &params, d_out_rgba8, out_len, hip_stream));
}
inline std::vector<MirtAdaptPixel> adapt_read(MirtContext* ctx)
{
    std::vector<MirtAdaptPixel> out((size_t)adapt_stats(ctx).pixels);
    MirtAdaptPixel none{};
    check(mirt_ctx_adapt_read(ctx, out.empty() ? &none : out.data(), out.size()));
    return out;
}
inline void adapt_write(MirtContext* ctx, const std::vector<MirtAdaptPixel>& records) { check(mirt_ctx_adapt_write(ctx, records.data(), records.size())); }
// the pixels the last step sampled: ascending places in the band
inline std::vector<uint32_t> adapt_list(MirtContext* ctx)
{
    std::vector<uint32_t> list((size_t)adapt_stats(ctx).pixels + 1u);
    uint32_t count = 0;
    check(mirt_ctx_adapt_list_read(ctx, list.data(), list.size(), &count));
    list.resize(count);
    return list;
}
// Adaptive runs (mirt_ctx_adapt_run_device): run.max_steps steps queued by one call on `hip_stream`, every step's sample count chosen on the
// device from the list it has just built.  adapt_run_spp is that rule for one count, host only; adapt_run_log blocks.
static_assert(sizeof(MirtAdaptRun) == 16 && sizeof(MirtAdaptRunStep) == 8 && MIRT_ADAPT_RUN_MAX_STEPS == 256u, "the adaptive run of include/mirt.h");
inline uint32_t adapt_run_spp(uint32_t count, uint32_t spp, const MirtAdaptRun& run)
{
    uint32_t out = 0;
    check(mirt_adapt_run_spp(count, spp, &run, &out));
    return out;
}
inline void adapt_run(MirtContext* ctx, const MirtParams& params, const MirtAdaptParams& adapt, const MirtAdaptRun& run, void* hip_stream = nullptr)
{
    check(mirt_ctx_adapt_run_device(ctx, &params, &adapt, &run, hip_stream));
}
// {count, spp} of every step of the last run
inline std::vector<MirtAdaptRunStep> adapt_run_log(MirtContext* ctx)
{
    std::vector<MirtAdaptRunStep> log(MIRT_ADAPT_RUN_MAX_STEPS);
    uint32_t n_steps = 0;
    check(mirt_ctx_adapt_run_read(ctx, log.data(), log.size(), &n_steps));
    log.resize(n_steps);
    return log;
}
// MIRT_ADAPT_LDS in MirtAdaptParams.flags: adapt_step and adapt_run also accept a scene that lives in LDS, where it stays (same records as on
// the same world held as a MIRT_SCENE_HBM scene, which ignores the flag).  adapt_lds_plan is the geometry such a step runs (grid_bytes =
// MirtGridPlan.blob_bytes, 0 for the flat layout; all fields 0: no such layout), adapt_lds_groups the rule by which the device deals a
// pixel's samples to 1 << g groups of lanes; both host only.
static_assert(MIRT_ADAPT_LDS == 1u << 3 && sizeof(MirtAdaptLdsPlan) == 16, "MirtAdaptParams.flags: adaptive steps on a scene in LDS");
// MIRT_QUERY_LDS in the flags of trace_rays / render_features and in MirtRadianceParams.flags: the query also accepts a scene that lives in
// LDS, where it stays (same records as on the same world held as a MIRT_SCENE_HBM scene, which ignores the flag); geometry: adapt_lds_plan.
constexpr uint32_t kQueryLds = MIRT_QUERY_LDS;
static_assert(kQueryLds == 1u << 8, "ray, feature and radiance queries on a scene in LDS");
inline MirtAdaptLdsPlan adapt_lds_plan(uint32_t n_spheres, uint32_t n_materials, uint32_t grid_bytes = 0, bool hosek = false, uint64_t lds_bytes_per_cu = 0)
{
    MirtAdaptLdsPlan plan;
    check(mirt_adapt_lds_plan(n_spheres, n_materials, grid_bytes, hosek ? 1u : 0u, lds_bytes_per_cu, &plan));
    return plan;
}
inline uint32_t adapt_lds_groups(uint32_t count, uint32_t spp, uint32_t grid_waves)
{
    uint32_t out = 0;
    check(mirt_adapt_lds_groups(count, spp, grid_waves, &out));
    return out;
}
// the pinhole ray through the centre of pixel (x, y), row 0 on top: cameraMakeRay with a zero lens
inline MirtRay pixel_ray(const MirtGpuCamera& cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float t_max = 1000.0f)
{
    const float u = ((float)x + 0.5f) / (float)width, v = 1.0f - ((float)y + 0.5f) / (float)height;
    MirtRay r{};
    for (int k = 0; k < 3; ++k) {
        r.origin[k] = cam.eye[k];
        r.direction[k] = (cam.lower_left_corner[k] + u * cam.horizontal[k] + v * cam.vertical[k]) - cam.eye[k];
    }
    r.t_max = t_max;
    return r;
}

// move_spheres of Layer / Raytracer: held[first ..] take centre and radius of `spheres` and keep their material
inline void move_held_spheres(std::vector<MirtSphere>& held, uint32_t first, const std::vector<MirtSphere>& spheres)
{
    if ((uint64_t)first + spheres.size() > held.size()) throw MirtError(MIRT_ERR_BAD_ROWS, "move_spheres: range beyond the scene's spheres");
    for (size_t i = 0; i < spheres.size(); ++i) {
        for (int k = 0; k < 4; ++k) held[first + i].center[k] = spheres[i].center[k];
        held[first + i].radius = spheres[i].radius;
    }
}

// Angle — angle.rs:1-50
class Angle {
    float radians_;
    explicit Angle(float r) : radians_(r) {}
public:
    static Angle degrees(float d) { return Angle(mirt_degrees_to_radians(d)); }
    static Angle radians(float r) { return Angle(r); }
    float as_degrees() const { return mirt_radians_to_degrees(radians_); }
    float as_radians() const { return radians_; }
    Angle clamp(Angle lo, Angle hi) const {
        float r = radians_;
        if (r < lo.radians_) r = lo.radians_;
        if (r > hi.radians_) r = hi.radians_;
        return Angle(r);
    }
    Angle operator+(Angle rhs) const { return Angle(radians_ + rhs.radians_); }
    bool operator==(Angle o) const { return radians_ == o.radians_; }
};

// Camera — mod.rs:489-499
struct Camera {
    Vec3 eye_pos, eye_dir, up;
    Angle vfov = Angle::degrees(30.0f);
    float aperture = 0.0f, focus_distance = 1.0f;
    MirtCamera to_c() const {
        return MirtCamera{ { eye_pos.x, eye_pos.y, eye_pos.z }, { eye_dir.x, eye_dir.y, eye_dir.z }, { up.x, up.y, up.z },
                           vfov.as_radians(), aperture, focus_distance };
    }
};

// SamplingParams — mod.rs:597-613
struct SamplingParams { uint32_t max_samples_per_pixel = 128, num_samples_per_pixel = 2, num_bounces = 8; };

// RenderParams — mod.rs:442-485
struct RenderParams {
    Camera camera;
    SamplingParams sampling;
    uint32_t viewport_w = 800, viewport_h = 600;
    void validate() const {
        const MirtCamera c = camera.to_c();
        const MirtSamplingParams s{ sampling.max_samples_per_pixel, sampling.num_samples_per_pixel, sampling.num_bounces };
        check(mirt_validate_render_params(&c, &s, viewport_w, viewport_h));
    }
};

// GpuCamera::new — mod.rs:700-741
inline MirtGpuCamera gpu_camera_new(const Camera& cam, uint32_t w, uint32_t h)
{
    MirtGpuCamera out;
    const MirtCamera c = cam.to_c();
    check(mirt_camera_new(&c, w, h, &out));
    return out;
}

// FlyCameraController::default + renderer_camera — fly_camera.rs:24-64
inline Camera default_fly_camera()
{
    const float pos[3] = { -10.0f, 2.0f, -4.0f };
    const float dx = 10.0f, dy = -1.0f, dz = 4.0f;                 // look_at - look_from
    const float focus = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    MirtCamera c;
    check(mirt_camera_from_fly_pose(pos, mirt_degrees_to_radians(25.0f), mirt_degrees_to_radians(-10.0f), 30.0f, 0.8f, focus, &c));
    Camera out;
    out.eye_pos = { c.eye_pos[0], c.eye_pos[1], c.eye_pos[2] };
    out.eye_dir = { c.eye_dir[0], c.eye_dir[1], c.eye_dir[2] };
    out.up = { c.up[0], c.up[1], c.up[2] };
    out.vfov = Angle::radians(c.vfov_radians);
    out.aperture = c.aperture;
    out.focus_distance = c.focus_distance;
    return out;
}

// Sphere::new — mod.rs:423-431
inline MirtSphere sphere_new(Vec3 center, float radius, uint32_t material_idx)
{
    return MirtSphere{ { center.x, center.y, center.z, 0.0f }, radius, material_idx, { 0u, 0u } };
}

// Texture — texture.rs:9-78.  Decoded RGB8 sources only (binary PPM "P6" or raw .rgb8 with explicit
// size): JPEG decoding belongs to the `image` crate on the Rust side and is not rebuilt here.
class Texture {
    uint32_t w_ = 0, h_ = 0;
    std::vector<float> data_;      // [w*h][3]
public:
    static Texture new_from_color(Vec3 c) { Texture t; t.w_ = t.h_ = 1; t.data_ = { c.x, c.y, c.z }; return t; }
    static Texture new_from_rgb8(const uint8_t* rgb, uint32_t w, uint32_t h) {
        Texture t; t.w_ = w; t.h_ = h; t.data_.resize((size_t)w * h * 3);
        const float inv_255 = 1.0f / 255.0f;                       // texture.rs:30
        for (size_t i = 0; i < t.data_.size(); ++i) t.data_[i] = inv_255 * (float)rgb[i];
        return t;
    }
    // texture.rs:21-46.  JPEG files (what the reference loads: assets/moon.jpeg, assets/earthmap.jpeg) go through the
    // library's own decoder (mirt_jpeg_decode_rgb8); binary PPM is accepted beside it for already-decoded texels.
    static Texture new_from_image(const std::string& path) {       // TextureError::FileIoError / ImageLoadError on failure
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("TextureError::IoError: cannot open " + path);
        if (f.peek() == 0xff) {
            std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            uint32_t jw = 0, jh = 0;
            if (mirt_jpeg_info(bytes.data(), bytes.size(), &jw, &jh) != MIRT_OK)
                throw std::runtime_error(std::string("TextureError::ImageLoadError: ") + mirt_jpeg_last_error() + ": " + path);
            std::vector<uint8_t> rgb((size_t)jw * jh * 3);
            if (mirt_jpeg_decode_rgb8(bytes.data(), bytes.size(), rgb.data(), rgb.size()) != MIRT_OK)
                throw std::runtime_error(std::string("TextureError::ImageLoadError: ") + mirt_jpeg_last_error() + ": " + path);
            return new_from_rgb8(rgb.data(), jw, jh);
        }
        std::string magic; uint32_t w = 0, h = 0, maxv = 0;
        f >> magic >> w >> h >> maxv;
        if (magic != "P6" || maxv != 255 || w == 0 || h == 0) throw std::runtime_error("TextureError::ImageLoadError: not a binary PPM: " + path);
        f.get();
        std::vector<uint8_t> rgb((size_t)w * h * 3);
        f.read(reinterpret_cast<char*>(rgb.data()), (std::streamsize)rgb.size());
        if ((size_t)f.gcount() != rgb.size()) throw std::runtime_error("TextureError::ImageLoadError: truncated " + path);
        return new_from_rgb8(rgb.data(), w, h);
    }
    const std::vector<float>& as_slice() const { return data_; }
    uint32_t width() const { return w_; }
    uint32_t height() const { return h_; }
};

// enum Material — mod.rs:433-438
struct Lambertian { Texture albedo; };
struct Metal { Texture albedo; float fuzz; };
struct Dielectric { float refraction_index; };
struct Checkerboard { Texture even, odd; };
using Material = std::variant<Lambertian, Metal, Dielectric, Checkerboard>;

struct Scene { std::vector<MirtSphere> spheres; std::vector<Material> materials; };

// GpuMaterial::* + append_to_global_texture_data — mod.rs:767-830
namespace gpu_material {
inline MirtTextureDescriptor empty() { return MirtTextureDescriptor{ 0u, 0u, 0xffffffffu }; }   // mod.rs:878-886
inline MirtTextureDescriptor append(const Texture& t, std::vector<float>& gtd) {
    const uint32_t offset = (uint32_t)(gtd.size() / 3);
    gtd.insert(gtd.end(), t.as_slice().begin(), t.as_slice().end());
    return MirtTextureDescriptor{ t.width(), t.height(), offset };
}
inline MirtMaterial lambertian(const Texture& a, std::vector<float>& g) { return MirtMaterial{ 0u, append(a, g), empty(), 0.0f }; }
inline MirtMaterial metal(const Texture& a, float fuzz, std::vector<float>& g) { return MirtMaterial{ 1u, append(a, g), empty(), fuzz }; }
inline MirtMaterial dielectric(float ior) { return MirtMaterial{ 2u, empty(), empty(), ior }; }
inline MirtMaterial checkerboard(const Texture& even, const Texture& odd, std::vector<float>& g) {
    const MirtTextureDescriptor d1 = append(even, g);
    const MirtTextureDescriptor d2 = append(odd, g);
    return MirtMaterial{ 3u, d1, d2, 0.0f };
}
}  // namespace gpu_material

// Layer — layer.rs:37-282 (imgui/wgpu upload paths are UI and out of scope)
class Layer {
public:
    float vp_size[2];
    MirtGpuCamera camera;
    std::vector<MirtSphere> world;          // Vec<Box<Sphere>> gathered contiguously
    std::vector<Material> materials;

    Layer(const float size[2], const RenderParams& rp, Scene scene, int device = 0)     // layer.rs:49-88
        : world(std::move(scene.spheres)), materials(std::move(scene.materials)), device_(device)
    {
        vp_size[0] = size[0]; vp_size[1] = size[1];
        camera = gpu_camera_new(rp.camera, (uint32_t)size[0], (uint32_t)size[1]);
    }
    ~Layer() { if (ctx_) mirt_ctx_destroy(ctx_); }
    Layer(const Layer&) = delete;
    Layer& operator=(const Layer&) = delete;

    // Layer::scene — layer.rs:90-123; the two image textures come from decoded files
    static Scene scene(const std::string& moon_ppm, const std::string& earth_ppm)
    {
        Scene s;
        s.materials.emplace_back(Checkerboard{ Texture::new_from_color({ 0.5f, 0.7f, 0.8f }), Texture::new_from_color({ 0.9f, 0.9f, 0.9f }) });
        s.materials.emplace_back(Lambertian{ Texture::new_from_image(moon_ppm) });
        s.materials.emplace_back(Metal{ Texture::new_from_color({ 1.0f, 0.85f, 0.57f }), 0.4f });
        s.materials.emplace_back(Dielectric{ 1.5f });
        s.materials.emplace_back(Lambertian{ Texture::new_from_image(earth_ppm) });
        s.spheres = { sphere_new({ 5.0f, 1.2f, -1.5f }, 1.2f, 4), sphere_new({ 0.0f, -500.0f, -1.0f }, 500.0f, 0),
                      sphere_new({ 0.0f, 1.0f, 0.0f }, 1.0f, 3),   sphere_new({ -5.0f, 1.0f, 0.0f }, 1.0f, 2),
                      sphere_new({ 2.0f, -1.0f, 0.0f }, 2.0f, 3),  sphere_new({ 5.0f, 0.8f, 1.5f }, 0.8f, 1) };
        return s;
    }

    // layer.rs:125-148; the call sites pass (odd, even) into a (even, odd) signature
    bool set_global_data()
    {
        material_data_.clear();
        global_texture_data_.clear();
        for (const Material& m : materials) {
            if (auto* l = std::get_if<Lambertian>(&m)) material_data_.push_back(gpu_material::lambertian(l->albedo, global_texture_data_));
            else if (auto* me = std::get_if<Metal>(&m)) material_data_.push_back(gpu_material::metal(me->albedo, me->fuzz, global_texture_data_));
            else if (auto* d = std::get_if<Dielectric>(&m)) material_data_.push_back(gpu_material::dielectric(d->refraction_index));
            else { const auto& c = std::get<Checkerboard>(m); material_data_.push_back(gpu_material::checkerboard(c.odd, c.even, global_texture_data_)); }
        }
        return true;
    }

    // layer.rs:264-282 — the hot path: one FFI call
    void set_data(const RenderParams& rp)
    {
        if (!ctx_) check(mirt_ctx_create(device_, &ctx_));
        upload(world);
        render(rp);
    }

    // Spheres first .. of `world` take centre and radius of `spheres` (they keep their material).  After a set_data whose world went to
    // device memory (MIRT_SCENE_HBM) the resident scene is updated in place and its BVH refitted; any other resident scene is set again;
    // before the first set_data only `world` changes.  With `rp` the image is rendered again, as set_data does.  `world` changes only
    // when the device call succeeded.
    void move_spheres(uint32_t first, const std::vector<MirtSphere>& spheres, const RenderParams* rp = nullptr)
    {
        std::vector<MirtSphere> moved = world;
        move_held_spheres(moved, first, spheres);
        if (ctx_ && hbm_) {
            const int rc = mirt_ctx_update_spheres(ctx_, first, (uint32_t)spheres.size(), spheres.data());
            if (rc != MIRT_OK && rc != MIRT_ERR_BAD_ROWS && rc != MIRT_ERR_NULL_POINTER) hbm_ = false;   // no scene any more: the next call sets one
            check(rc);
        } else if (ctx_) {
            upload(moved);
        }
        world.swap(moved);
        if (ctx_ && rp) render(*rp);
    }

    // `world` becomes `spheres` (any count, their material indices taken).  A resident MIRT_SCENE_HBM scene gets the new sphere table in
    // place (mirt_ctx_set_spheres); any other resident scene is set again; before the first set_data only `world` changes.  With `rp` the
    // image is rendered again.  `world` changes only when the device call succeeded.
    void set_world(const std::vector<MirtSphere>& spheres, const RenderParams* rp = nullptr)
    {
        std::vector<MirtSphere> next = spheres;
        if (ctx_ && hbm_) {
            const int rc = mirt_ctx_set_spheres(ctx_, next.data(), (uint32_t)next.size());
            if (rc != MIRT_OK && rc != MIRT_ERR_SCENE_TOO_LARGE && rc != MIRT_ERR_NULL_POINTER) hbm_ = false;   // no scene any more: the next call sets one
            check(rc);
        } else if (ctx_) {
            upload(next);
        }
        world.swap(next);
        if (ctx_ && rp) render(*rp);
    }

    // layer.rs:182-186: ImageBuffer<Rgb<u8>> view
    std::vector<uint8_t> imgbuf() const
    {
        std::vector<uint8_t> rgb(rgba_.size() / 4 * 3);
        if (!rgba_.empty()) check(mirt_rgba8_to_rgb8(rgba_.data(), rgba_.size() / 4, rgb.data()));
        return rgb;
    }
    const std::vector<uint8_t>& register_texture() const { return rgba_; }    // the RGBA8 bytes imgui would get (layer.rs:150-176)
    void update_camera(const RenderParams& rp) { camera = gpu_camera_new(rp.camera, rp.viewport_w, rp.viewport_h); }   // layer.rs:188-193
    void resize(const RenderParams& rp)                                        // layer.rs:240-262
    {
        if (vp_size[0] != (float)rp.viewport_w || vp_size[1] != (float)rp.viewport_h) {
            vp_size[0] = (float)rp.viewport_w; vp_size[1] = (float)rp.viewport_h;
            update_camera(rp);
            set_data(rp);
        }
    }
    const std::vector<MirtMaterial>& material_data() const { return material_data_; }
    const std::vector<float>& global_texture_data() const { return global_texture_data_; }

    MirtContext* context() const { return ctx_; }      // nullptr before the first set_data

private:
    void upload(const std::vector<MirtSphere>& spheres)
    {
        MirtScene sc{};
        sc.camera = &camera;
        sc.spheres = spheres.data(); sc.n_spheres = (uint32_t)spheres.size();
        sc.materials = material_data_.data(); sc.n_materials = (uint32_t)material_data_.size();
        sc.texels = global_texture_data_.data(); sc.n_texels = global_texture_data_.size() / 3;
        hbm_ = false;
        check(set_scene_any_size(ctx_, sc, &hbm_));        // a world beyond the LDS budget: MIRT_SCENE_HBM
    }
    void render(const RenderParams& rp)
    {
        const uint32_t w = (uint32_t)vp_size[0], h = (uint32_t)vp_size[1];
        MirtParams p{};
        p.width = w; p.height = h; p.spp = rp.sampling.num_samples_per_pixel; p.mode = MIRT_MODE_PARITY;
        rgba_.assign((size_t)w * h * 4, 0);
        check(mirt_ctx_render(ctx_, &p, rgba_.data(), rgba_.size()));
    }
    int device_;
    MirtContext* ctx_ = nullptr;
    bool hbm_ = false;                                   // ctx_ holds a MIRT_SCENE_HBM scene
    std::vector<MirtMaterial> material_data_;
    std::vector<float> global_texture_data_;
    std::vector<uint8_t> rgba_;
};

// Node — one frame on several devices (mirt_node_*): member contexts on `devices`, the parts assembled on member 0.  Same
// device everywhere -> loopback; all distinct (or rccl = true) -> RCCL gather.  Throws MirtError like the rest of the mirror.
class Node {
public:
    explicit Node(const std::vector<int>& devices, bool rccl = false)
    {
        check(mirt_node_create(devices.data(), (uint32_t)devices.size(), rccl ? (uint32_t)MIRT_NODE_RCCL : 0u, &node_));
    }
    ~Node() { if (node_) mirt_node_destroy(node_); }
    Node(const Node&) = delete;
    Node& operator=(const Node&) = delete;
    Node(Node&& o) noexcept : node_(o.node_) { o.node_ = nullptr; }
    Node& operator=(Node&& o) noexcept
    {
        if (this != &o) { if (node_) mirt_node_destroy(node_); node_ = o.node_; o.node_ = nullptr; }
        return *this;
    }

    void set_scene(const MirtScene& scene) { check(mirt_node_set_scene(node_, &scene)); }
    // flags: MIRT_SCENE_* (mirt_node_set_scene_ex)
    void set_scene(const MirtScene& scene, uint32_t flags) { check(mirt_node_set_scene_ex(node_, &scene, flags)); }
    void set_camera(const MirtGpuCamera& camera) { check(mirt_node_set_camera(node_, &camera)); }
    // the band of `p` (tile_rows = n_parts = part = 0) as RGBA8, blocking
    std::vector<uint8_t> render(const MirtParams& p)
    {
        std::vector<uint8_t> out((size_t)mirt_params_out_rows(&p) * p.width * 4);
        check(mirt_node_render(node_, &p, out.data(), out.size()));
        return out;
    }
    // asynchronous, into device memory on member 0's device, ordered on `hip_stream` (nullptr: the node's own stream)
    void render_device(const MirtParams& p, void* d_out_rgba8, size_t out_len, void* hip_stream = nullptr)
    {
        check(mirt_node_render_device(node_, &p, d_out_rgba8, out_len, hip_stream));
    }
    // ---- progressive accumulation: every member owns the exact sums of its part; a frame moves RGBA8 parts only ----
    void accum_reset(const MirtParams& p) { check(mirt_node_accum_reset(node_, &p)); }
    // one progressive frame of the band (p.spp further samples; 0 = the mean of what is there), blocking
    std::vector<uint8_t> accum_frame(const MirtParams& p)
    {
        std::vector<uint8_t> out((size_t)mirt_params_out_rows(&p) * p.width * 4);
        check(mirt_node_accum_frame(node_, &p, out.data(), out.size()));
        return out;
    }
    void accum_frame_device(const MirtParams& p, void* d_out_rgba8, size_t out_len, void* hip_stream = nullptr)
    {
        check(mirt_node_accum_frame_device(node_, &p, d_out_rgba8, out_len, hip_stream));
    }
    uint32_t accum_samples() const { return mirt_node_accum_samples(node_); }
    std::vector<uint64_t> accum_read(const MirtParams& p)          // band-row order, pixels x 3
    {
        std::vector<uint64_t> out((size_t)mirt_params_out_rows(&p) * p.width * 3);
        check(mirt_node_accum_read(node_, out.data(), out.size()));
        return out;
    }
    MirtContext* context(uint32_t i) const            // borrowed: the node owns it
    {
        MirtContext* c = nullptr;
        check(mirt_node_context(node_, i, &c));
        return c;
    }
    MirtNodeStats stats() const
    {
        MirtNodeStats s{};
        check(mirt_node_get_stats(node_, &s));
        return s;
    }
    MirtNode* raw() const { return node_; }

private:
    MirtNode* node_ = nullptr;
};

// Raytracer — the path-traced mode behind the names of src/raytracer/mod.rs:20-394 (wgpu plumbing
// omitted).  render_frame() = RenderProgress::next_frame (mod.rs:626-670) + the shader's accumulation: ONE frame call.
// With a device LIST the loop runs through a node (mirt_node_accum_*): every frame cut across the members; the images are the same.
class Raytracer {
public:
    Raytracer(const Scene& scene, const RenderParams& rp, int device = 0, const MirtSkyState* sky = nullptr)
        : rp_(rp), spheres_(scene.spheres)
    {
        init(scene, sky);
        check(mirt_ctx_create(device, &ctx_));
        upload();
    }
    Raytracer(const Scene& scene, const RenderParams& rp, const std::vector<int>& devices, const MirtSkyState* sky = nullptr)
        : rp_(rp), spheres_(scene.spheres)
    {
        init(scene, sky);
        check(mirt_node_create(devices.data(), (uint32_t)devices.size(), 0u, &node_));
        upload();
    }
    ~Raytracer() { if (ctx_) mirt_ctx_destroy(ctx_); if (node_) mirt_node_destroy(node_); }
    Raytracer(const Raytracer&) = delete;
    Raytracer& operator=(const Raytracer&) = delete;

    void set_render_params(const RenderParams& rp)                         // mod.rs:353-388
    {
        rp.validate();
        rp_ = rp;
        camera_ = gpu_camera_new(rp.camera, rp.viewport_w, rp.viewport_h);
        check(node_ ? mirt_node_set_camera(node_, &camera_) : mirt_ctx_set_camera(ctx_, &camera_));
        accumulated_ = -1;                                                 // render_progress.reset()
    }

    // Spheres first .. of the scene take centre and radius of `spheres` (they keep their material): in place, with a refit of the BVH, when
    // the scene is in device memory (MIRT_SCENE_HBM); any other scene is set again.  The accumulation restarts (render_progress.reset()).
    // The held spheres change only when the device call succeeded.
    void move_spheres(uint32_t first, const std::vector<MirtSphere>& spheres)
    {
        std::vector<MirtSphere> moved = spheres_;
        move_held_spheres(moved, first, spheres);
        if (hbm_) {
            const int rc = node_ ? mirt_node_update_spheres(node_, first, (uint32_t)spheres.size(), spheres.data())
                                 : mirt_ctx_update_spheres(ctx_, first, (uint32_t)spheres.size(), spheres.data());
            if (rc != MIRT_OK && rc != MIRT_ERR_BAD_ROWS && rc != MIRT_ERR_NULL_POINTER) hbm_ = false;   // no scene any more: the next call sets one
            check(rc);
            spheres_.swap(moved);
        } else {
            spheres_.swap(moved);
            try { upload(); } catch (...) { spheres_.swap(moved); throw; }
        }
        accumulated_ = -1;
    }

    // The scene's spheres become `spheres` (any count, their material indices taken): in place, with a tree built on the device, when the
    // scene is in device memory (MIRT_SCENE_HBM); any other scene is set again.  The accumulation restarts.  The held spheres change only
    // when the device call succeeded.
    void set_world(const std::vector<MirtSphere>& spheres)
    {
        std::vector<MirtSphere> next = spheres;
        if (hbm_) {
            const int rc = node_ ? mirt_node_set_spheres(node_, next.data(), (uint32_t)next.size())
                                 : mirt_ctx_set_spheres(ctx_, next.data(), (uint32_t)next.size());
            if (rc != MIRT_OK && rc != MIRT_ERR_SCENE_TOO_LARGE && rc != MIRT_ERR_NULL_POINTER) hbm_ = false;   // no scene any more: the next call sets one
            check(rc);
            spheres_.swap(next);
        } else {
            spheres_.swap(next);
            try { upload(); } catch (...) { spheres_.swap(next); throw; }
        }
        accumulated_ = -1;
    }

    // all max_samples_per_pixel samples in one launch
    std::vector<uint8_t> render(uint64_t seed = 0, uint32_t flags = 0)
    {
        MirtParams p = params(rp_.sampling.max_samples_per_pixel, seed, flags);
        std::vector<uint8_t> out((size_t)p.width * p.height * 4);
        check(node_ ? mirt_node_render(node_, &p, out.data(), out.size()) : mirt_ctx_render(ctx_, &p, out.data(), out.size()));
        return out;
    }

    // one progressive frame, one call: add num_samples_per_pixel until max_samples_per_pixel (then spp = 0: the mean of what is
    // there, mod.rs:350), return the estimate
    std::vector<uint8_t> render_frame(uint64_t seed = 0, uint32_t flags = 0)
    {
        MirtParams p = next_frame(seed, flags);
        std::vector<uint8_t> out((size_t)p.width * p.height * 4);
        check(node_ ? mirt_node_accum_frame(node_, &p, out.data(), out.size()) : mirt_ctx_accum_frame(ctx_, &p, out.data(), out.size()));
        accumulated_ += (int)p.spp;
        return out;
    }
    // the same frame into device memory (height x width x 4 bytes), asynchronously on `hip_stream` (nullptr: the context's / node's
    // own stream): for hosts that draw from device memory.  Two frames in flight: alternate the streams of mirt_ctx_frame_stream
    // and two framebuffers.
    void render_frame_device(void* d_out_rgba8, void* hip_stream = nullptr, uint64_t seed = 0, uint32_t flags = 0)
    {
        MirtParams p = next_frame(seed, flags);
        const size_t len = (size_t)p.width * p.height * 4;
        check(node_ ? mirt_node_accum_frame_device(node_, &p, d_out_rgba8, len, hip_stream)
                    : mirt_ctx_accum_frame_device(ctx_, &p, d_out_rgba8, len, hip_stream));
        accumulated_ += (int)p.spp;
    }
    float progress() const { return (accumulated_ < 0 ? 0.0f : (float)accumulated_) / (float)rp_.sampling.max_samples_per_pixel; }   // mod.rs:390-393
    MirtContext* context() const { return ctx_; }      // nullptr when the loop runs on a node
    MirtNode* node() const { return node_; }

private:
    // RenderProgress::next_frame: clears after a reset; the params of the frame call to issue now
    MirtParams next_frame(uint64_t seed, uint32_t flags)
    {
        MirtParams p = params(rp_.sampling.num_samples_per_pixel, seed, flags);
        if (accumulated_ < 0) { check(node_ ? mirt_node_accum_reset(node_, &p) : mirt_ctx_accum_reset(ctx_, &p)); accumulated_ = 0; }
        if ((uint32_t)accumulated_ + p.spp > rp_.sampling.max_samples_per_pixel) p.spp = 0;
        return p;
    }
    void init(const Scene& scene, const MirtSkyState* sky)
    {
        const RenderParams& rp = rp_;
        rp.validate();                                                     // mod.rs:44-47
        for (const Material& m : scene.materials) {                        // mod.rs:160-183 (same (odd, even) swap)
            if (auto* l = std::get_if<Lambertian>(&m)) material_data_.push_back(gpu_material::lambertian(l->albedo, texels_));
            else if (auto* me = std::get_if<Metal>(&m)) material_data_.push_back(gpu_material::metal(me->albedo, me->fuzz, texels_));
            else if (auto* d = std::get_if<Dielectric>(&m)) material_data_.push_back(gpu_material::dielectric(d->refraction_index));
            else { const auto& c = std::get<Checkerboard>(m); material_data_.push_back(gpu_material::checkerboard(c.odd, c.even, texels_)); }
        }
        if (sky) { sky_ = *sky; have_sky_ = true; }
        camera_ = gpu_camera_new(rp.camera, rp.viewport_w, rp.viewport_h);
    }
    MirtParams params(uint32_t spp, uint64_t seed, uint32_t flags) const
    {
        MirtParams p{};
        p.width = rp_.viewport_w; p.height = rp_.viewport_h; p.spp = spp; p.num_bounces = rp_.sampling.num_bounces;
        p.mode = MIRT_MODE_PT; p.flags = flags | (have_sky_ ? (uint32_t)MIRT_FLAG_SKY_HOSEK : 0u); p.seed = seed;
        return p;
    }
    void upload()
    {
        MirtScene sc{};
        sc.camera = &camera_;
        sc.spheres = spheres_.data(); sc.n_spheres = (uint32_t)spheres_.size();
        sc.materials = material_data_.data(); sc.n_materials = (uint32_t)material_data_.size();
        sc.texels = texels_.data(); sc.n_texels = texels_.size() / 3;
        sc.sky = have_sky_ ? &sky_ : nullptr;
        if (node_) {                                       // a world beyond the LDS budget: MIRT_SCENE_HBM
            int rc = mirt_node_set_scene(node_, &sc);
            hbm_ = rc == MIRT_ERR_SCENE_TOO_LARGE;
            if (hbm_) rc = mirt_node_set_scene_ex(node_, &sc, MIRT_SCENE_HBM);
            check(rc);
        } else {
            check(set_scene_any_size(ctx_, sc, &hbm_));
        }
    }
    RenderParams rp_;
    std::vector<MirtSphere> spheres_;
    std::vector<MirtMaterial> material_data_;
    std::vector<float> texels_;
    MirtGpuCamera camera_{};
    MirtSkyState sky_{};
    bool have_sky_ = false;
    MirtContext* ctx_ = nullptr;
    MirtNode* node_ = nullptr;
    int accumulated_ = -1;
    bool hbm_ = false;                                   // the context / node holds a MIRT_SCENE_HBM scene
};

}  // namespace mirt_host
