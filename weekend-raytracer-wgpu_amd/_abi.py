"""ctypes mirror of include/mirt.h — the C ABI of the MI355X ray-trace path.

Every struct here is byte-identical to the header (and therefore to the reference's
`#[repr(C)]` Rust types cited there).  tests/test_abi.py checks sizes and offsets.
"""
from __future__ import annotations

import ctypes as C

MIRT_MODE_PARITY = 0
MIRT_MODE_PT = 1
MIRT_MAX_SPP_PER_CALL = 1 << 24

MIRT_FLAG_SKY_HOSEK = 1 << 0
MIRT_FLAG_NO_TONEMAP = 1 << 1
MIRT_FLAG_NO_SRGB = 1 << 2
MIRT_FLAG_COUNT_WORK = 1 << 3
MIRT_FLAG_KERNEL_STRIP = 1 << 4
MIRT_FLAG_KERNEL_POOL = 1 << 5
MIRT_FLAG_NO_GRID = 1 << 6
MIRT_FLAG_COUNT_GRID = 1 << 7
MIRT_FLAG_FAST_MATH = 1 << 8
MIRT_FLAG_TEXEL_TILES = 1 << 9

# mirt_ctx_set_scene_ex / mirt_node_set_scene_ex flags, and the BVH of such scenes
MIRT_SCENE_HBM = 1 << 0
MIRT_SCENE_BVH_DEVICE = 1 << 1       # only together with MIRT_SCENE_HBM: build the BVH on the device
MIRT_SCENE_HBM_MAX_SPHERES = 1 << 24
MIRT_BVH_MAX_DEPTH = 32
MIRT_BVH_MAX_LEAF = 4
MIRT_BVH_MAX_ALWAYS = 64
MIRT_BVH_BIG_RADII = 4

# mirt_ctx_trace_rays* flags, and the `sphere` of a ray that hits nothing
MIRT_RAYS_FLAT = 1 << 0
MIRT_RAYS_ANY_HIT = 1 << 1
MIRT_RAYS_COUNT = 1 << 2
MIRT_RAYS_SORT = 1 << 4                 # bit 3 is unassigned
MIRT_RAY_MISS = 0xFFFFFFFF

# mirt_ctx_render_features* flags
MIRT_FEATURES_FLAT = 1 << 0

# mirt_ctx_trace_radiance* flags (MirtRadianceParams.flags)
MIRT_RADIANCE_FLAT = 1 << 0
MIRT_RADIANCE_ACCUMULATE = 1 << 1
MIRT_RADIANCE_SKY_HOSEK = 1 << 2
MIRT_RADIANCE_SORT = 1 << 4             # bit 3 is unassigned
MIRT_RADIANCE_POOL = 1 << 6             # bit 5 is unassigned
# the sort code of MIRT_RAYS_SORT / MIRT_RADIANCE_SORT: bits per origin axis / per octahedral direction axis
MIRT_RAY_SORT_ORIGIN_BITS = 5
MIRT_RAY_SORT_DIRECTION_BITS = 8

# mirt_ctx_adapt_*: the rule's floor, 0.125 of radiance per sample summed over the channels, in 2^-20 units
MIRT_ADAPT_FLOOR = 1 << 17
MIRT_ADAPT_POOL = 1 << 1                # MirtAdaptParams.flags; bit 0 is unassigned
MIRT_ADAPT_LDS = 1 << 3                 # MirtAdaptParams.flags: a step also runs on a scene that lives in LDS; bit 2 is unassigned
MIRT_QUERY_LDS = 1 << 8                 # the flags of mirt_ctx_trace_rays*, mirt_ctx_render_features* and MirtRadianceParams.flags: the query also runs on a scene that lives in LDS
MIRT_ADAPT_RUN_MAX_STEPS = 256          # mirt_ctx_adapt_run_device: steps of one run, entries of its log

# mirt_ctx_denoise*: MirtDenoiseParams.source and MirtDenoiseParams.flags
MIRT_DENOISE_SRC_ACCUM = 0
MIRT_DENOISE_SRC_ADAPT = 1
MIRT_DENOISE_OUT_F32 = 1 << 0

# mirt_ctx_reproject*: MirtReprojectParams.flags
MIRT_REPROJECT_CLAMP = 1 << 0

# mirt_node_create: members at most, and its flags
MIRT_NODE_MAX_MEMBERS = 16
MIRT_NODE_RCCL = 1 << 0

MIRT_OK = 0
STATUS = {
    0: "MIRT_OK",
    -1: "MIRT_ERR_MAX_SAMPLES_MULTIPLE",
    -2: "MIRT_ERR_VIEWPORT_SIZE",
    -3: "MIRT_ERR_VFOV_RANGE",
    -4: "MIRT_ERR_APERTURE_RANGE",
    -5: "MIRT_ERR_FOCUS_DISTANCE",
    -6: "MIRT_ERR_SKY",
    -10: "MIRT_ERR_NULL_POINTER",
    -11: "MIRT_ERR_SPP_ZERO",
    -12: "MIRT_ERR_BAD_MODE",
    -13: "MIRT_ERR_BAD_ROWS",
    -14: "MIRT_ERR_MATERIAL_INDEX",
    -15: "MIRT_ERR_TEXEL_RANGE",
    -16: "MIRT_ERR_OUT_BUFFER",
    -17: "MIRT_ERR_NO_SCENE",
    -18: "MIRT_ERR_SCENE_TOO_LARGE",
    -19: "MIRT_ERR_FRAME_SPP",
    -20: "MIRT_ERR_NO_DEVICE",
    -21: "MIRT_ERR_HIP",
    -22: "MIRT_ERR_ALLOC",
    -23: "MIRT_ERR_IMAGE_DECODE",
    -24: "MIRT_ERR_SPP_RANGE",
}
for _code, _name in STATUS.items():
    globals()[_name] = _code


class MirtSphere(C.Structure):
    _fields_ = [("center", C.c_float * 4), ("radius", C.c_float),
                ("material_idx", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class MirtTextureDescriptor(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("offset", C.c_uint32)]


class MirtMaterial(C.Structure):
    _fields_ = [("id", C.c_uint32), ("desc1", MirtTextureDescriptor),
                ("desc2", MirtTextureDescriptor), ("x", C.c_float)]


class MirtGpuCamera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("_padding1", C.c_float),
                ("horizontal", C.c_float * 3), ("_padding2", C.c_float),
                ("vertical", C.c_float * 3), ("_padding3", C.c_float),
                ("u", C.c_float * 3), ("_padding4", C.c_float),
                ("v", C.c_float * 3), ("lens_radius", C.c_float),
                ("lower_left_corner", C.c_float * 3), ("_padding5", C.c_float)]


class MirtSkyState(C.Structure):
    _fields_ = [("params", C.c_float * 27), ("radiances", C.c_float * 3),
                ("_padding", C.c_uint32 * 2), ("sun_direction", C.c_float * 4)]


class MirtCamera(C.Structure):
    _fields_ = [("eye_pos", C.c_float * 3), ("eye_dir", C.c_float * 3), ("up", C.c_float * 3),
                ("vfov_radians", C.c_float), ("aperture", C.c_float), ("focus_distance", C.c_float)]


class MirtSamplingParams(C.Structure):
    _fields_ = [("max_samples_per_pixel", C.c_uint32), ("num_samples_per_pixel", C.c_uint32),
                ("num_bounces", C.c_uint32)]


class MirtScene(C.Structure):
    _fields_ = [("camera", C.POINTER(MirtGpuCamera)),
                ("spheres", C.POINTER(MirtSphere)), ("n_spheres", C.c_uint32),
                ("materials", C.POINTER(MirtMaterial)), ("n_materials", C.c_uint32),
                ("texels", C.POINTER(C.c_float)), ("n_texels", C.c_uint64),
                ("sky", C.POINTER(MirtSkyState))]


class MirtParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32),
                ("num_bounces", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32),
                ("seed", C.c_uint64), ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
                ("tile_rows", C.c_uint32), ("n_parts", C.c_uint32), ("part", C.c_uint32),
                ("sample_begin", C.c_uint32), ("frame_spp", C.c_uint32), ("frame_begin", C.c_uint32)]


class MirtGridPlan(C.Structure):
    _fields_ = [("cell_factor", C.c_float), ("blob_bytes", C.c_uint32), ("n_cells", C.c_uint32), ("n_entries", C.c_uint32),
                ("n_big", C.c_uint32), ("pool_slots", C.c_uint32)]


class MirtBvhPlan(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("n_leaf_spheres", C.c_uint32), ("n_always", C.c_uint32),
                ("max_depth", C.c_uint32), ("max_leaf", C.c_uint32), ("device_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MirtBvhInfo(C.Structure):
    _fields_ = [("plan", MirtBvhPlan), ("root", C.c_uint32), ("built_on_device", C.c_uint32),
                ("centre", C.c_float * 3), ("radius", C.c_float), ("r_max", C.c_float)]

    def as_dict(self) -> dict:
        return {"plan": self.plan.as_dict(), "root": int(self.root), "built_on_device": int(self.built_on_device),
                "centre": [float(v) for v in self.centre], "radius": float(self.radius), "r_max": float(self.r_max)}


class MirtBvhPoolPlan(C.Structure):
    _fields_ = [("threads", C.c_uint32), ("slots", C.c_uint32), ("waves_per_cu", C.c_uint32), ("stack_entries", C.c_uint32),
                ("lds_bytes_per_block", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MirtStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("kernel_ms_total", C.c_double), ("launches", C.c_uint64),
                ("samples", C.c_uint64), ("rays", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("roots", C.c_uint64), ("hits", C.c_uint64),
                ("scatter", C.c_uint64 * 5), ("sky_misses", C.c_uint64),
                ("lane_iterations", C.c_uint64), ("wave_iterations", C.c_uint64),
                ("grid_cells", C.c_uint64), ("grid_wave_cells", C.c_uint64),
                ("texel_fetches", C.c_uint64 * 2), ("texel_tile_hits", C.c_uint64 * 2)]

    def as_dict(self) -> dict:
        return {"kernel_ms": self.kernel_ms, "kernel_ms_total": self.kernel_ms_total, "launches": self.launches,
                "samples": self.samples, "rays": self.rays,
                "sphere_tests": self.sphere_tests, "roots": self.roots, "hits": self.hits,
                "scatter": list(self.scatter), "sky_misses": self.sky_misses,
                "lane_iterations": self.lane_iterations, "wave_iterations": self.wave_iterations,
                "grid_cells": self.grid_cells, "grid_wave_cells": self.grid_wave_cells,
                "texel_fetches": list(self.texel_fetches), "texel_tile_hits": list(self.texel_tile_hits)}


class MirtRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("_pad", C.c_float)]


class MirtRayHit(C.Structure):
    _fields_ = [("t", C.c_float), ("sphere", C.c_uint32), ("point", C.c_float * 3), ("normal", C.c_float * 3)]


class MirtFeaturePixel(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("t", C.c_float), ("normal", C.c_float * 3), ("sphere", C.c_uint32)]


class MirtRadianceRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("stream", C.c_uint32), ("direction", C.c_float * 3), ("_pad", C.c_uint32)]


class MirtRadiance(C.Structure):
    _fields_ = [("sum", C.c_uint64 * 3), ("samples", C.c_uint32), ("_pad", C.c_uint32)]


class MirtRadianceParams(C.Structure):
    _fields_ = [("spp", C.c_uint32), ("sample_begin", C.c_uint32), ("num_bounces", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64)]


class MirtAdaptPixel(C.Structure):
    _fields_ = [("sum", C.c_uint64 * 3), ("even", C.c_uint64 * 3), ("samples", C.c_uint32), ("_pad0", C.c_uint32), ("_pad1", C.c_uint64)]


class MirtAdaptParams(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("tolerance", C.c_uint32), ("flags", C.c_uint32)]


class MirtAdaptRun(C.Structure):
    _fields_ = [("max_steps", C.c_uint32), ("min_items", C.c_uint32), ("max_spp", C.c_uint32), ("flags", C.c_uint32)]


class MirtAdaptRunStep(C.Structure):
    _fields_ = [("count", C.c_uint32), ("spp", C.c_uint32)]


class MirtAdaptLdsPlan(C.Structure):
    _fields_ = [("threads", C.c_uint32), ("grid", C.c_uint32), ("lds_bytes_per_block", C.c_uint32), ("blocks_per_cu", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MirtDenoiseParams(C.Structure):
    _fields_ = [("source", C.c_uint32), ("levels", C.c_uint32), ("normal_log2", C.c_uint32), ("flags", C.c_uint32), ("sigma_colour", C.c_float),
                ("_pad", C.c_uint32 * 3)]


class MirtReprojectParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("max_history", C.c_float), ("depth_tolerance", C.c_float), ("_pad", C.c_uint32),
                ("previous", MirtGpuCamera), ("current", MirtGpuCamera)]


class MirtReprojectFrames(C.Structure):
    _fields_ = [("colour", C.c_void_p), ("guides", C.c_void_p), ("prev_colour", C.c_void_p), ("prev_guides", C.c_void_p), ("out", C.c_void_p),
                ("out_rgba8", C.c_void_p), ("pixels", C.c_uint64)]


class MirtAdaptStats(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("total_samples", C.c_uint64), ("active", C.c_uint32), ("steps", C.c_uint32), ("kernel_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "total_samples": int(self.total_samples), "active": int(self.active), "steps": int(self.steps),
                "kernel_ms": self.kernel_ms}


class MirtRayStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("rays", C.c_uint64), ("sphere_tests", C.c_uint64), ("roots", C.c_uint64),
                ("hits", C.c_uint64), ("nodes", C.c_uint64), ("wave_nodes", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"kernel_ms": self.kernel_ms, **{k: int(getattr(self, k)) for k, _ in self._fields_[1:]}}


class MirtNodeStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("transport", C.c_uint32), ("gather_ms", C.c_double), ("assemble_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {"n_members": self.n_members, "transport": self.transport, "gather_ms": self.gather_ms,
                "assemble_ms": self.assemble_ms}


# every symbol include/mirt.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "mirt_version": (C.c_uint32, []),
    "mirt_last_error": (C.c_char_p, []),
    "mirt_status_string": (C.c_char_p, [C.c_int]),
    "mirt_validate_render_params": (C.c_int, [_P(MirtCamera), _P(MirtSamplingParams), C.c_uint32, C.c_uint32]),
    "mirt_camera_new": (C.c_int, [_P(MirtCamera), C.c_uint32, C.c_uint32, _P(MirtGpuCamera)]),
    "mirt_camera_from_fly_pose": (C.c_int, [_P(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                            C.c_float, _P(MirtCamera)]),
    "mirt_degrees_to_radians": (C.c_float, [C.c_float]),
    "mirt_radians_to_degrees": (C.c_float, [C.c_float]),
    "mirt_params_out_rows": (C.c_uint32, [_P(MirtParams)]),
    "mirt_params_out_row_index": (C.c_uint32, [_P(MirtParams), C.c_uint32]),
    "mirt_grid_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, _P(MirtGridPlan)]),
    "mirt_ctx_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "mirt_ctx_destroy": (None, [C.c_void_p]),
    "mirt_ctx_set_scene": (C.c_int, [C.c_void_p, _P(MirtScene)]),
    "mirt_ctx_set_scene_ex": (C.c_int, [C.c_void_p, _P(MirtScene), C.c_uint32]),
    "mirt_bvh_plan": (C.c_int, [C.c_void_p, C.c_uint32, _P(MirtBvhPlan)]),
    "mirt_ctx_bvh_info": (C.c_int, [C.c_void_p, _P(MirtBvhInfo)]),
    "mirt_bvh_pool_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, _P(MirtBvhPoolPlan)]),
    "mirt_adapt_pool_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, _P(MirtBvhPoolPlan)]),
    "mirt_ctx_bvh_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "mirt_ctx_update_spheres": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mirt_ctx_update_spheres_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mirt_ctx_set_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mirt_ctx_set_spheres_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mirt_ctx_bvh_refits": (C.c_uint32, [C.c_void_p]),
    "mirt_ctx_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mirt_ctx_trace_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mirt_ctx_trace_stats": (C.c_int, [C.c_void_p, _P(MirtRayStats)]),
    "mirt_ctx_render_features": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_uint32, C.c_void_p, C.c_size_t]),
    "mirt_ctx_render_features_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_camera_pixel_ray": (C.c_int, [_P(MirtGpuCamera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P(MirtRay)]),
    "mirt_ctx_trace_radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _P(MirtRadianceParams), C.c_void_p]),
    "mirt_ctx_trace_radiance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _P(MirtRadianceParams), C.c_void_p, C.c_void_p]),
    "mirt_ray_sort_code": (C.c_int, [_P(C.c_float), C.c_float, C.c_void_p, _P(C.c_uint32)]),
    "mirt_ctx_trace_order_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mirt_ctx_set_camera": (C.c_int, [C.c_void_p, _P(MirtGpuCamera)]),
    "mirt_ctx_render": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_ctx_render_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_ctx_last_kernel": (C.c_char_p, [C.c_void_p]),
    "mirt_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "mirt_ctx_get_stats": (C.c_int, [C.c_void_p, _P(MirtStats)]),
    "mirt_ctx_accum_reset": (C.c_int, [C.c_void_p, _P(MirtParams)]),
    "mirt_ctx_accum_add": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p]),
    "mirt_ctx_accum_samples": (C.c_uint32, [C.c_void_p]),
    "mirt_ctx_accum_resolve": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_ctx_accum_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mirt_ctx_accum_frame_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_ctx_accum_frame": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_adapt_active": (C.c_int, [_P(MirtAdaptPixel), _P(MirtAdaptParams), _P(C.c_uint32)]),
    "mirt_ctx_adapt_reset": (C.c_int, [C.c_void_p, _P(MirtParams)]),
    "mirt_ctx_adapt_step_device": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtAdaptParams), C.c_void_p]),
    "mirt_ctx_adapt_resolve_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_ctx_adapt_resolve": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_ctx_adapt_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mirt_ctx_adapt_write": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mirt_ctx_adapt_list_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_uint32)]),
    "mirt_ctx_adapt_stats": (C.c_int, [C.c_void_p, _P(MirtAdaptStats)]),
    "mirt_adapt_run_spp": (C.c_int, [C.c_uint32, C.c_uint32, _P(MirtAdaptRun), _P(C.c_uint32)]),
    "mirt_ctx_denoise_device": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtDenoiseParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_ctx_denoise": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtDenoiseParams), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "mirt_ctx_reproject_device": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtReprojectParams), _P(MirtReprojectFrames), C.c_void_p]),
    "mirt_ctx_reproject": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtReprojectParams), _P(MirtReprojectFrames)]),
    "mirt_camera_project": (C.c_int, [_P(MirtGpuCamera), C.c_uint32, C.c_uint32, _P(C.c_float), _P(C.c_float)]),
    "mirt_adapt_lds_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, _P(MirtAdaptLdsPlan)]),
    "mirt_adapt_lds_groups": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint32)]),
    "mirt_ctx_adapt_run_device": (C.c_int, [C.c_void_p, _P(MirtParams), _P(MirtAdaptParams), _P(MirtAdaptRun), C.c_void_p]),
    "mirt_ctx_adapt_run_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_uint32)]),
    "mirt_ctx_selftest_math": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "mirt_ctx_selftest_checker_sign": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "mirt_ctx_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "mirt_ctx_frame_stream": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mirt_render": (C.c_int, [_P(MirtScene), _P(MirtParams), C.c_int, C.c_void_p, C.c_size_t]),
    "mirt_rgba8_to_rgb8": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_jpeg_info": (C.c_int, [C.c_void_p, C.c_size_t, _P(C.c_uint32), _P(C.c_uint32)]),
    "mirt_jpeg_decode_rgb8": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "mirt_rgb8_to_texels": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_jpeg_last_error": (C.c_char_p, []),
    "mirt_ctx_deinterleave_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_node_create": (C.c_int, [_P(C.c_int), C.c_uint32, C.c_uint32, _P(C.c_void_p)]),
    "mirt_node_destroy": (None, [C.c_void_p]),
    "mirt_node_set_scene": (C.c_int, [C.c_void_p, _P(MirtScene)]),
    "mirt_node_set_scene_ex": (C.c_int, [C.c_void_p, _P(MirtScene), C.c_uint32]),
    "mirt_node_update_spheres": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mirt_node_set_spheres": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mirt_node_set_camera": (C.c_int, [C.c_void_p, _P(MirtGpuCamera)]),
    "mirt_node_render": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_node_render_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_node_context": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_void_p)]),
    "mirt_node_get_stats": (C.c_int, [C.c_void_p, _P(MirtNodeStats)]),
    "mirt_node_accum_reset": (C.c_int, [C.c_void_p, _P(MirtParams)]),
    "mirt_node_accum_frame_device": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "mirt_node_accum_frame": (C.c_int, [C.c_void_p, _P(MirtParams), C.c_void_p, C.c_size_t]),
    "mirt_node_accum_samples": (C.c_uint32, [C.c_void_p]),
    "mirt_node_accum_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
}


def bind(lib: C.CDLL, symbols: dict = SYMBOLS) -> None:
    """Attach restype/argtypes; raises AttributeError if the library lacks a declared symbol."""
    for name, (restype, argtypes) in symbols.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
