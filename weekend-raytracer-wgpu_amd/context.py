"""Thin object wrappers over the C ABI: SceneData (the bytes a `Layer` holds) and Context
(one per GPU: resident scene + render calls).  All compute happens behind libmirt.so."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._lib import MirtError, check, lib


@dataclass
class SceneData:
    """What `Layer` holds when `set_data` runs (reference src/raytracer/layer.rs:37-46), flattened
    to the wire format: GpuCamera, contiguous spheres, GpuMaterial table, [f32;3] texel table."""
    camera: _abi.MirtGpuCamera
    spheres: Sequence[_abi.MirtSphere]
    materials: Sequence[_abi.MirtMaterial]
    texels: np.ndarray                       # float32 [n_texels, 3]
    sky: Optional[_abi.MirtSkyState] = None

    def __post_init__(self) -> None:
        self.texels = np.ascontiguousarray(self.texels, dtype=np.float32).reshape(-1, 3)
        self._c_spheres = (_abi.MirtSphere * max(1, len(self.spheres)))(*self.spheres)
        self._c_mats = (_abi.MirtMaterial * max(1, len(self.materials)))(*self.materials)

    def as_c(self) -> _abi.MirtScene:
        s = _abi.MirtScene()
        s.camera = C.pointer(self.camera)
        s.spheres = C.cast(self._c_spheres, C.POINTER(_abi.MirtSphere))
        s.n_spheres = len(self.spheres)
        s.materials = C.cast(self._c_mats, C.POINTER(_abi.MirtMaterial))
        s.n_materials = len(self.materials)
        s.texels = self.texels.ctypes.data_as(C.POINTER(C.c_float)) if self.texels.size else None
        s.n_texels = self.texels.shape[0]
        s.sky = C.pointer(self.sky) if self.sky is not None else None
        return s


def make_params(width: int, height: int, spp: int, *, mode: int = _abi.MIRT_MODE_PARITY, num_bounces: int = 8,
                flags: int = 0, seed: int = 0, row_begin: int = 0, row_end: int = 0, tile_rows: int = 0,
                n_parts: int = 0, part: int = 0, sample_begin: int = 0, frame_spp: int = 0, frame_begin: int = 0) -> _abi.MirtParams:
    p = _abi.MirtParams()
    p.width, p.height, p.spp, p.num_bounces = width, height, spp, num_bounces
    p.mode, p.flags, p.seed = mode, flags, seed
    p.row_begin, p.row_end = row_begin, row_end
    p.tile_rows, p.n_parts, p.part, p.sample_begin = tile_rows, n_parts, part, sample_begin
    p.frame_spp = frame_spp
    p.frame_begin = frame_begin
    return p


def set_scene_any_size(target, scene: SceneData) -> bool:
    """`target.set_scene(scene)` (a Context or a Node); a world the LDS layouts refuse (MIRT_ERR_SCENE_TOO_LARGE) is set again with
    MIRT_SCENE_HBM, so that the reference's host objects -- `Layer::set_data` takes any `Vec<Box<Sphere>>` -- take any world."""
    try:
        target.set_scene(scene)
    except MirtError as e:
        if e.status != _abi.MIRT_ERR_SCENE_TOO_LARGE:
            raise
        target.set_scene(scene, hbm=True)
        return True                          # an HBM scene: its spheres can be moved in place (update_spheres)
    return False


def bvh_plan(spheres) -> dict:
    """mirt_bvh_plan: the BVH mirt_ctx_set_scene_ex(MIRT_SCENE_HBM) would build over `spheres` (a sequence of MirtSphere or a
    ctypes array of them), host only."""
    n = len(spheres)
    arr = spheres if isinstance(spheres, C.Array) else (_abi.MirtSphere * max(1, n))(*spheres)
    out = _abi.MirtBvhPlan()
    check(lib().mirt_bvh_plan(C.cast(arr, C.c_void_p), n, C.byref(out)))
    return out.as_dict()


def bvh_pool_plan(max_depth: int, hosek: bool = False, lds_bytes_per_cu: int = 0) -> dict:
    """mirt_bvh_pool_plan: the geometry MIRT_FLAG_KERNEL_POOL runs on a MIRT_SCENE_HBM scene whose tree is `max_depth` deep
    (Context.bvh_info()["plan"]["max_depth"]), host only: {"threads", "slots", "waves_per_cu", "stack_entries",
    "lds_bytes_per_block"}; slots == 0: none fits and the launch runs the strip kernel.  lds_bytes_per_cu = 0: gfx950's 163 840."""
    out = _abi.MirtBvhPoolPlan()
    check(lib().mirt_bvh_pool_plan(int(max_depth), 1 if hosek else 0, int(lds_bytes_per_cu), C.byref(out)))
    return out.as_dict()


def adapt_pool_plan(max_depth: int, hosek: bool = False, lds_bytes_per_cu: int = 0) -> dict:
    """mirt_adapt_pool_plan: the geometry an adaptive step with MIRT_ADAPT_POOL runs on a MIRT_SCENE_HBM scene whose tree is `max_depth`
    deep, host only: the dict of bvh_pool_plan, with the 512 bytes per wave the pooled step keeps beside its pool; slots == 0: none fits
    and the step runs as without the flag.  lds_bytes_per_cu = 0: gfx950's 163 840."""
    out = _abi.MirtBvhPoolPlan()
    check(lib().mirt_adapt_pool_plan(int(max_depth), 1 if hosek else 0, int(lds_bytes_per_cu), C.byref(out)))
    return out.as_dict()


def adapt_lds_plan(n_spheres: int, n_materials: int, grid_bytes: int = 0, hosek: bool = False, lds_bytes_per_cu: int = 0) -> dict:
    """mirt_adapt_lds_plan: the geometry an adaptive step with MIRT_ADAPT_LDS runs on a scene that lives in LDS, host only: {"threads",
    "grid", "lds_bytes_per_block", "blocks_per_cu"}.  grid_bytes = grid_plan()["blob_bytes"] for the grid layout, 0 for the flat one; all
    fields 0: a layout the render launches refuse.  lds_bytes_per_cu = 0: gfx950's 163 840."""
    for name, v in (("n_spheres", n_spheres), ("n_materials", n_materials), ("grid_bytes", grid_bytes)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    out = _abi.MirtAdaptLdsPlan()
    check(lib().mirt_adapt_lds_plan(int(n_spheres), int(n_materials), int(grid_bytes), 1 if hosek else 0, int(lds_bytes_per_cu), C.byref(out)))
    return out.as_dict()


def adapt_lds_groups(count: int, spp: int, grid_waves: int) -> int:
    """mirt_adapt_lds_groups: log2 of the sample groups an MIRT_ADAPT_LDS step deals a pixel's `spp` samples to when it lists `count`
    pixels and its grid has `grid_waves` waves -- the function every wave runs on the device.  Needs no device."""
    for name, v in (("count", count), ("spp", spp), ("grid_waves", grid_waves)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    out = C.c_uint32()
    check(lib().mirt_adapt_lds_groups(int(count), int(spp), int(grid_waves), C.byref(out)))
    return int(out.value)


# one inner node as mirt_ctx_bvh_read returns it (csrc/mirt_bvh.h: BvhNode, 64 bytes)
BVH_NODE_DTYPE = np.dtype([("lmin", "<f4", (3,)), ("lmax", "<f4", (3,)), ("rmin", "<f4", (3,)), ("rmax", "<f4", (3,)),
                           ("left", "<u4"), ("right", "<u4"), ("pad", "<u4", (2,))])
BVH_LEAF = 0x80000000      # a child reference with this bit is a leaf: bits 24..30 = sphere count, bits 0..23 = first record


def scene_flags(hbm: bool, bvh: str) -> int:
    """The mirt_*_set_scene_ex flags of `set_scene(scene, hbm=..., bvh=...)`: bvh = "host" (default) or "device"
    (MIRT_SCENE_BVH_DEVICE, only with hbm=True)."""
    if bvh not in ("host", "device"):
        raise ValueError(f"bvh must be 'host' or 'device', not {bvh!r}")
    if bvh == "device" and not hbm:
        raise ValueError("bvh='device' needs hbm=True (MIRT_SCENE_BVH_DEVICE only together with MIRT_SCENE_HBM)")
    return (_abi.MIRT_SCENE_HBM if hbm else 0) | (_abi.MIRT_SCENE_BVH_DEVICE if bvh == "device" else 0)


# MirtSphere as a numpy record (32 bytes): what update_spheres takes for large worlds
SPHERE_DTYPE = np.dtype([("center", "<f4", (4,)), ("radius", "<f4"), ("material_idx", "<u4"), ("_pad", "<u4", (2,))])


def sphere_records(spheres) -> tuple:
    """`spheres` for the update_spheres wrappers -> (address, count, keep-alive object): a one-dimensional SPHERE_DTYPE numpy array, a
    ctypes array of MirtSphere or a list / tuple of Sphere (anything with to_c() -> MirtSphere) or MirtSphere.  Anything else:
    ValueError, before the library is called."""
    if isinstance(spheres, np.ndarray):
        if spheres.dtype != SPHERE_DTYPE or spheres.ndim != 1:
            raise ValueError(f"spheres must be a one-dimensional SPHERE_DTYPE array, not {spheres.dtype} of shape {spheres.shape}")
        arr = np.ascontiguousarray(spheres)
        return C.c_void_p(arr.ctypes.data if len(arr) else None), len(arr), arr
    if isinstance(spheres, C.Array):
        if spheres._type_ is not _abi.MirtSphere:
            raise ValueError(f"spheres must be a ctypes array of MirtSphere, not of {spheres._type_.__name__}")
        return C.cast(spheres, C.c_void_p), len(spheres), spheres
    if isinstance(spheres, (list, tuple)):
        recs = [s if isinstance(s, _abi.MirtSphere) else s.to_c() if hasattr(s, "to_c") else None for s in spheres]
        if not all(isinstance(s, _abi.MirtSphere) for s in recs):
            raise ValueError("spheres must hold Sphere / MirtSphere records only")
        arr = (_abi.MirtSphere * max(1, len(recs)))(*recs)
        return C.cast(arr, C.c_void_p), len(spheres), arr
    raise ValueError(f"spheres must be a SPHERE_DTYPE array, a ctypes MirtSphere array or a list of Sphere, not {type(spheres).__name__}")


# MirtRay / MirtRayHit as numpy records (32 bytes each): what trace_rays takes and returns
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("direction", "<f4", (3,)), ("_pad", "<f4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("sphere", "<u4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,))])
RAYS_FLAGS = _abi.MIRT_RAYS_FLAT | _abi.MIRT_RAYS_ANY_HIT | _abi.MIRT_RAYS_COUNT | _abi.MIRT_RAYS_SORT


def make_rays(origins, directions, t_max=1000.0) -> np.ndarray:
    """A RAY_DTYPE array from origins [n, 3] (or one origin), directions [n, 3] and t_max (a scalar or [n]); 1000 is the renderer's
    own bound (MAX_T)."""
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    rays = np.zeros(len(d), RAY_DTYPE)
    rays["origin"] = np.asarray(origins, np.float32)
    rays["direction"] = d
    rays["t_max"] = np.asarray(t_max, np.float32)
    return rays


def ray_records(rays) -> np.ndarray:
    """`rays` for trace_rays -> a contiguous one-dimensional RAY_DTYPE array (a view where possible): a RAY_DTYPE array, or a float32
    array [n, 8] = {origin, t_max, direction, pad} (bit patterns are kept).  Anything else: ValueError, before the library is called."""
    if not isinstance(rays, np.ndarray):
        raise ValueError(f"rays must be a numpy array of RAY_DTYPE or float32 [n, 8], not {type(rays).__name__}")
    if rays.dtype == RAY_DTYPE and rays.ndim == 1:
        return np.ascontiguousarray(rays)
    if rays.dtype == np.float32 and rays.ndim == 2 and rays.shape[1] == 8:
        return np.ascontiguousarray(rays).view(RAY_DTYPE).reshape(-1)
    raise ValueError(f"rays must be a one-dimensional RAY_DTYPE array or float32 [n, 8], not {rays.dtype} of shape {rays.shape}")


def _lds_flag(lds) -> int:
    """MIRT_QUERY_LDS for lds=True: the query also runs on a scene that lives in LDS, where it stays (an HBM scene ignores it)."""
    if not isinstance(lds, (bool, np.bool_)):
        raise ValueError(f"lds must be a bool, not {lds!r}")
    return _abi.MIRT_QUERY_LDS if lds else 0


def _check_rays_flags(flags, sort=False, lds=False) -> int:
    if not isinstance(flags, (int, np.integer)) or isinstance(flags, bool) or int(flags) & ~RAYS_FLAGS or int(flags) < 0:
        raise ValueError(f"flags must be a combination of MIRT_RAYS_FLAT, MIRT_RAYS_ANY_HIT, MIRT_RAYS_COUNT and MIRT_RAYS_SORT, not {flags!r}")
    if not isinstance(sort, (bool, np.bool_)):
        raise ValueError(f"sort must be a bool, not {sort!r}")
    return int(flags) | (_abi.MIRT_RAYS_SORT if sort else 0) | _lds_flag(lds)


def ray_sort_codes(centre, radius, rays) -> np.ndarray:
    """mirt_ray_sort_code for every record of `rays` (a RAY_DTYPE or RADIANCE_RAY_DTYPE array: both keep the origin at byte 0 and the
    direction at byte 16) -> uint32 [n], the 31-bit codes a sorted launch orders by; centre, radius: those of Context.bvh_info().
    Needs no device."""
    if not isinstance(rays, np.ndarray) or rays.dtype not in (RAY_DTYPE, RADIANCE_RAY_DTYPE) or rays.ndim != 1:
        raise ValueError("rays must be a one-dimensional RAY_DTYPE or RADIANCE_RAY_DTYPE array")
    cen = np.asarray(centre, np.float32)
    if cen.shape != (3,):
        raise ValueError(f"centre must hold three floats, not shape {cen.shape}")
    if not isinstance(radius, (int, float, np.integer, np.floating)) or isinstance(radius, bool):
        raise ValueError(f"radius must be a number, not {radius!r}")
    recs = np.ascontiguousarray(rays)
    cen = np.ascontiguousarray(cen)
    codes = np.zeros(len(recs), np.uint32)
    f, code = lib().mirt_ray_sort_code, C.c_uint32()
    c_cen, c_rad = cen.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(float(np.float32(radius)))
    for i in range(len(recs)):
        check(f(c_cen, c_rad, C.c_void_p(recs.ctypes.data + 32 * i), C.byref(code)))
        codes[i] = code.value
    return codes


def _check_address(name, v) -> int:
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or int(v) <= 0:
        raise ValueError(f"{name} must be a device address, not {v!r}")
    return int(v)


# MirtFeaturePixel as a numpy record (32 bytes): what render_features returns per pixel
FEATURE_DTYPE = np.dtype([("albedo", "<f4", (3,)), ("t", "<f4"), ("normal", "<f4", (3,)), ("sphere", "<u4")])


def make_denoise_params(source="accum", *, levels: int = 3, sigma_colour: float = 1.0, normal_log2: int = 5, f32: bool = False) -> _abi.MirtDenoiseParams:
    """MirtDenoiseParams for Context.denoise*: source "accum" (the accumulation buffer) or "adapt" (the adaptive records); `levels`
    a-trous levels (1..8), the colour weight's sigma (0: no colour weight), the normal weight's exponent as a power of two (0..8);
    f32=True asks for the linear mean as float32 RGBA instead of RGBA8.  The types are checked here, the ranges by the library."""
    if source not in ("accum", "adapt"):
        raise ValueError(f'source must be "accum" or "adapt", not {source!r}')
    for name, v in (("levels", levels), ("normal_log2", normal_log2)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < 2 ** 32:
            raise ValueError(f"{name} must be an unsigned integer, not {v!r}")
    if not isinstance(sigma_colour, (int, float, np.integer, np.floating)) or isinstance(sigma_colour, bool):
        raise ValueError(f"sigma_colour must be a number, not {sigma_colour!r}")
    if not isinstance(f32, (bool, np.bool_)):
        raise ValueError(f"f32 must be a bool, not {f32!r}")
    d = _abi.MirtDenoiseParams()
    d.source = _abi.MIRT_DENOISE_SRC_ADAPT if source == "adapt" else _abi.MIRT_DENOISE_SRC_ACCUM
    d.levels, d.normal_log2, d.flags = int(levels), int(normal_log2), _abi.MIRT_DENOISE_OUT_F32 if f32 else 0
    d.sigma_colour = float(sigma_colour)
    return d


def _check_denoise(denoise) -> _abi.MirtDenoiseParams:
    if not isinstance(denoise, _abi.MirtDenoiseParams):
        raise ValueError(f"denoise must be a MirtDenoiseParams (make_denoise_params builds one), not {type(denoise).__name__}")
    return denoise


def make_reproject_params(previous: _abi.MirtGpuCamera, current: _abi.MirtGpuCamera, *, max_history: float = 4.0, depth_tolerance: float = 0.05,
                          clamp: bool = True) -> _abi.MirtReprojectParams:
    """MirtReprojectParams for Context.reproject*: the cameras the previous and the current guide frame were taken with, the longest
    history a pixel may carry (the blend weight of the new frame is 1 / min(length + 1, max_history)), the relative depth tolerance
    of a tap, and whether the history is clamped to the colours of the pixel's 3 x 3 neighbourhood.  The types are checked here, the
    ranges by the library."""
    for name, v in (("previous", previous), ("current", current)):
        if not isinstance(v, _abi.MirtGpuCamera):
            raise ValueError(f"{name} must be a MirtGpuCamera, not {type(v).__name__}")
    for name, v in (("max_history", max_history), ("depth_tolerance", depth_tolerance)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool):
            raise ValueError(f"{name} must be a number, not {v!r}")
    if not isinstance(clamp, (bool, np.bool_)):
        raise ValueError(f"clamp must be a bool, not {clamp!r}")
    r = _abi.MirtReprojectParams()
    r.flags = _abi.MIRT_REPROJECT_CLAMP if clamp else 0
    r.max_history, r.depth_tolerance = float(np.float32(max_history)), float(np.float32(depth_tolerance))
    C.memmove(C.byref(r.previous), C.byref(previous), C.sizeof(_abi.MirtGpuCamera))
    C.memmove(C.byref(r.current), C.byref(current), C.sizeof(_abi.MirtGpuCamera))
    return r


def _check_reproject(reproject) -> _abi.MirtReprojectParams:
    if not isinstance(reproject, _abi.MirtReprojectParams):
        raise ValueError(f"reproject must be a MirtReprojectParams (make_reproject_params builds one), not {type(reproject).__name__}")
    return reproject


def camera_project(camera: _abi.MirtGpuCamera, w: int, h: int, point) -> np.ndarray:
    """mirt_camera_project: where `point` (three floats) falls in a w x h viewport of `camera` -> float32 [3] = {fx, fy, s}: pixel
    coordinates with pixel centres at integers and row 0 on top, and the parameter of the point along the pixel's centre ray
    (s > 0: in front of the camera).  The inverse of camera_pixel_ray up to rounding.  Needs no device."""
    if not isinstance(camera, _abi.MirtGpuCamera):
        raise ValueError(f"camera must be a MirtGpuCamera, not {type(camera).__name__}")
    for name, v in (("w", w), ("h", h)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    try:
        pt = np.array(point, np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"point must be three numbers, not {point!r}") from None
    if pt.shape != (3,):
        raise ValueError(f"point must be three numbers, not {point!r}")
    out = np.zeros(3, np.float32)
    fp = C.POINTER(C.c_float)
    check(lib().mirt_camera_project(C.byref(camera), int(w), int(h), pt.ctypes.data_as(fp), out.ctypes.data_as(fp)))
    return out


def _check_params(params) -> _abi.MirtParams:
    if not isinstance(params, _abi.MirtParams):
        raise ValueError(f"params must be a MirtParams (make_params builds one), not {type(params).__name__}")
    return params


def camera_pixel_ray(camera: _abi.MirtGpuCamera, w: int, h: int, x: int, y: int) -> np.ndarray:
    """mirt_camera_pixel_ray: the CENTRE ray of pixel (x, y) of a w x h viewport (row 0 on top) exactly as the feature kernel traces
    it -- float32 with fmaf, origin = eye, the lens ignored, t_max = 1000 -> one RAY_DTYPE record (a [1] array: what trace_rays takes).
    Needs no device.  A zero size or a pixel outside the viewport: MirtError."""
    if not isinstance(camera, _abi.MirtGpuCamera):
        raise ValueError(f"camera must be a MirtGpuCamera, not {type(camera).__name__}")
    for name, v in (("w", w), ("h", h), ("x", x), ("y", y)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    ray = np.zeros(1, RAY_DTYPE)
    check(lib().mirt_camera_pixel_ray(C.byref(camera), int(w), int(h), int(x), int(y), C.cast(C.c_void_p(ray.ctypes.data), C.POINTER(_abi.MirtRay))))
    return ray


# MirtRadianceRay / MirtRadiance as numpy records (32 bytes each): what trace_radiance takes and returns
RADIANCE_RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("stream", "<u4"), ("direction", "<f4", (3,)), ("_pad", "<u4")])
RADIANCE_DTYPE = np.dtype([("sum", "<u8", (3,)), ("samples", "<u4"), ("_pad", "<u4")])


def make_radiance_rays(origins, directions, streams=None) -> np.ndarray:
    """A RADIANCE_RAY_DTYPE array from origins [n, 3] (or one origin), directions [n, 3] (used as given, not normalised) and the
    rays' RNG streams (a scalar or [n] of u32; default: the ray's index, the place a pixel's index has in a render)."""
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    rays = np.zeros(len(d), RADIANCE_RAY_DTYPE)
    rays["origin"] = np.asarray(origins, np.float32)
    rays["direction"] = d
    st = np.arange(len(d), dtype=np.uint64) if streams is None else np.asarray(streams)
    if st.dtype.kind not in "iu" or (st.size and (int(st.min()) < 0 or int(st.max()) > 0xffffffff)):
        raise ValueError("streams must be integers in [0, 2^32)")
    rays["stream"] = st.astype(np.uint32)
    return rays


def radiance_ray_records(rays) -> np.ndarray:
    """`rays` for trace_radiance -> a contiguous one-dimensional RADIANCE_RAY_DTYPE array (a view where possible): a RADIANCE_RAY_DTYPE
    array, or a uint32 array [n, 8] of the records' bit patterns.  Anything else: ValueError, before the library is called."""
    if not isinstance(rays, np.ndarray):
        raise ValueError(f"rays must be a numpy array of RADIANCE_RAY_DTYPE or uint32 [n, 8], not {type(rays).__name__}")
    if rays.dtype == RADIANCE_RAY_DTYPE and rays.ndim == 1:
        return np.ascontiguousarray(rays)
    if rays.dtype == np.uint32 and rays.ndim == 2 and rays.shape[1] == 8:
        return np.ascontiguousarray(rays).view(RADIANCE_RAY_DTYPE).reshape(-1)
    raise ValueError(f"rays must be a one-dimensional RADIANCE_RAY_DTYPE array or uint32 [n, 8], not {rays.dtype} of shape {rays.shape}")


# MirtAdaptPixel as a numpy record (64 bytes): what adapt_read returns and adapt_write takes
ADAPT_PIXEL_DTYPE = np.dtype([("sum", "<u8", (3,)), ("even", "<u8", (3,)), ("samples", "<u4"), ("_pad0", "<u4"), ("_pad1", "<u8")])


def make_adapt_params(min_samples: int, max_samples: int, tolerance: int, pool: bool = False, lds: bool = False) -> _abi.MirtAdaptParams:
    """MirtAdaptParams: a pixel is sampled while it holds fewer than max_samples and either fewer than min_samples or its even and odd
    halves differ by more than tolerance x 2^-16 of its mean (include/mirt.h has the exact rule).  pool=True (MIRT_ADAPT_POOL): a hint
    to run the step's render stage on the pooled schedule; the records, the list and the counters are the same.  lds=True
    (MIRT_ADAPT_LDS): the step also runs on a scene that lives in LDS, where it stays; an HBM scene ignores it."""
    if not isinstance(pool, (bool, np.bool_)):
        raise ValueError(f"pool must be a bool, not {pool!r}")
    if not isinstance(lds, (bool, np.bool_)):
        raise ValueError(f"lds must be a bool, not {lds!r}")
    for name, v in (("min_samples", min_samples), ("max_samples", max_samples), ("tolerance", tolerance)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    a = _abi.MirtAdaptParams()
    a.min_samples, a.max_samples, a.tolerance, a.flags = int(min_samples), int(max_samples), int(tolerance), (_abi.MIRT_ADAPT_POOL if pool else 0) | (_abi.MIRT_ADAPT_LDS if lds else 0)
    return a


def adapt_active(records, adapt: _abi.MirtAdaptParams) -> np.ndarray:
    """mirt_adapt_active for every record of an ADAPT_PIXEL_DTYPE array -> bool [n]: the rule a step's select stage evaluates on the
    device.  Needs no device."""
    if not isinstance(records, np.ndarray) or records.dtype != ADAPT_PIXEL_DTYPE:
        raise ValueError("records must be an ADAPT_PIXEL_DTYPE array")
    if not isinstance(adapt, _abi.MirtAdaptParams):
        raise ValueError(f"adapt must be a MirtAdaptParams (make_adapt_params builds one), not {type(adapt).__name__}")
    recs = np.ascontiguousarray(records).reshape(-1)
    out = np.zeros(len(recs), bool)
    f, flag = lib().mirt_adapt_active, C.c_uint32()
    for i in range(len(recs)):
        check(f(C.cast(C.c_void_p(recs.ctypes.data + 64 * i), C.POINTER(_abi.MirtAdaptPixel)), C.byref(adapt), C.byref(flag)))
        out[i] = flag.value != 0
    return out.reshape(records.shape)


def make_adapt_run(max_steps: int, min_items: int = 0, max_spp: int = 0) -> _abi.MirtAdaptRun:
    """MirtAdaptRun for Context.adapt_run: `max_steps` steps (1 .. MIRT_ADAPT_RUN_MAX_STEPS) queued by one call.  A step that lists `count`
    pixels takes spp << k samples of each, k the smallest for which count x (spp << k) reaches `min_items` or spp << k is `max_spp`
    (0: params.spp, i.e. steps never grow; otherwise params.spp << m).  min_items = 0 never grows (include/mirt.h has the rule)."""
    for name, v in (("max_steps", max_steps), ("min_items", min_items), ("max_spp", max_spp)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    r = _abi.MirtAdaptRun()
    r.max_steps, r.min_items, r.max_spp, r.flags = int(max_steps), int(min_items), int(max_spp), 0
    return r


def adapt_run_spp(count: int, spp: int, run: _abi.MirtAdaptRun) -> int:
    """mirt_adapt_run_spp: the sample count a step of `run` takes when it lists `count` pixels and params.spp is `spp` -- the function
    the scan stage runs on the device.  Needs no device."""
    if not isinstance(run, _abi.MirtAdaptRun):
        raise ValueError(f"run must be a MirtAdaptRun (make_adapt_run builds one), not {type(run).__name__}")
    for name, v in (("count", count), ("spp", spp)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    out = C.c_uint32()
    check(lib().mirt_adapt_run_spp(int(count), int(spp), C.byref(run), C.byref(out)))
    return int(out.value)


def _radiance_params(spp, sample_begin, num_bounces, seed, flat, hosek, accumulate, sort=False, pool=False, lds=False) -> _abi.MirtRadianceParams:
    for name, v in (("spp", spp), ("sample_begin", sample_begin), ("num_bounces", num_bounces)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), not {seed!r}")
    for name, v in (("flat", flat), ("hosek", hosek), ("accumulate", accumulate), ("sort", sort), ("pool", pool)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, not {v!r}")
    flags = (_abi.MIRT_RADIANCE_FLAT if flat else 0) | (_abi.MIRT_RADIANCE_SKY_HOSEK if hosek else 0) | (_abi.MIRT_RADIANCE_ACCUMULATE if accumulate else 0) \
        | (_abi.MIRT_RADIANCE_SORT if sort else 0) | (_abi.MIRT_RADIANCE_POOL if pool else 0) | _lds_flag(lds)
    return _abi.MirtRadianceParams(int(spp), int(sample_begin), int(num_bounces), flags, int(seed))


def radiance_mean(records: np.ndarray) -> np.ndarray:
    """RADIANCE_DTYPE records -> float64 means [n, 3]: sum / 2^20 / samples (0 where a record holds no sample)."""
    n = np.maximum(records["samples"].astype(np.float64), 1.0)[:, None]
    return records["sum"].astype(np.float64) / float(1 << 20) / n


def _check_range(first, count) -> None:
    for name, v in (("first", first), ("count", count)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an integer in [0, 2^32), not {v!r}")


def params_out_rows(params: _abi.MirtParams) -> int:
    return int(lib().mirt_params_out_rows(C.byref(params)))


def params_out_row_index(params: _abi.MirtParams, i: int) -> int:
    return int(lib().mirt_params_out_row_index(C.byref(params), i))


HIP_STREAM_LEGACY = 1      # hipStreamLegacy ((hipStream_t)1, hip_runtime_api.h): the default ("null") stream by handle


def _stream_arg(stream: Optional[int]):
    """`stream` of the *_device / accum_add wrappers -> the C ABI's void* hip_stream.

    None  -> NULL: the context's own (non-blocking) stream.
    int h -> that hipStream_t; h == 0 is the DEFAULT stream (what `torch.cuda.current_stream().cuda_stream`
             returns unless a side stream is current) and is passed as hipStreamLegacy, because a NULL pointer
             already means "the context's own stream" in the C ABI -- sending 0 through would silently move the
             work to a stream that nothing the caller queues afterwards (an RCCL collective, a D2H copy) waits for."""
    if stream is None:
        return None
    return C.c_void_p(int(stream) if int(stream) != 0 else HIP_STREAM_LEGACY)


class Context:
    """mirt_ctx_* : one per HIP device; owns the device-resident scene."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().mirt_ctx_create(device, C.byref(self._h)))
        self.device = device
        self._scene: Optional[SceneData] = None

    def close(self) -> None:
        if self._h:
            lib().mirt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self) -> "Context":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, scene: SceneData, *, hbm: bool = False, bvh: str = "host") -> None:
        """mirt_ctx_set_scene; hbm=True: mirt_ctx_set_scene_ex(MIRT_SCENE_HBM) -- the tables stay in device memory and a BVH finds
        the nearest hit, for worlds beyond the LDS budget (any size up to MIRT_SCENE_HBM_MAX_SPHERES).  bvh="device" (with
        hbm=True): MIRT_SCENE_BVH_DEVICE, the tree is built on the device -- the same image, a much shorter call on large worlds."""
        flags = scene_flags(hbm, bvh)
        c = scene.as_c()
        if flags:
            check(lib().mirt_ctx_set_scene_ex(self._h, C.byref(c), flags))
        else:
            check(lib().mirt_ctx_set_scene(self._h, C.byref(c)))
        self._scene = scene
        self._scene_hbm = bool(hbm)

    def bvh_info(self) -> dict:
        """mirt_ctx_bvh_info: the tree this context holds -- {"plan": counts as bvh_plan() reports them, "root", "built_on_device",
        "centre", "radius", "r_max"}."""
        out = _abi.MirtBvhInfo()
        check(lib().mirt_ctx_bvh_info(self._h, C.byref(out)))
        return out.as_dict()

    def bvh_read(self) -> tuple:
        """mirt_ctx_bvh_read: (nodes [n_nodes] of BVH_NODE_DTYPE, recs float32 [n, 4] = {centre, r * r}, ids uint32 [n]) of the tree
        this context holds; blocking, meant for tests."""
        plan = self.bvh_info()["plan"]
        n = plan["n_leaf_spheres"] + plan["n_always"]
        nodes = np.zeros(plan["n_nodes"], BVH_NODE_DTYPE)
        recs = np.zeros((n, 4), np.float32)
        ids = np.zeros(n, np.uint32)
        check(lib().mirt_ctx_bvh_read(self._h, nodes.ctypes.data_as(C.c_void_p), nodes.nbytes, recs.ctypes.data_as(C.c_void_p), recs.size,
                                      ids.ctypes.data_as(C.c_void_p), ids.size))
        return nodes, recs, ids

    def update_spheres(self, first: int, spheres) -> None:
        """mirt_ctx_update_spheres: spheres first .. first + len(spheres) of the MIRT_SCENE_HBM scene take centre and radius from
        `spheres` (see sphere_records; material_idx is not read), the tree is refitted on the device.  Blocking."""
        ptr, count, keep = sphere_records(spheres)
        _check_range(first, count)
        check(lib().mirt_ctx_update_spheres(self._h, int(first), count, ptr))
        del keep

    def update_spheres_device(self, first: int, count: int, d_ptr: int) -> None:
        """mirt_ctx_update_spheres_device: the same from `count` 32-byte MirtSphere records in memory of this context's device at
        address `d_ptr` (e.g. a torch tensor's data_ptr(); what was queued to produce them is waited for)."""
        _check_range(first, count)
        if not isinstance(d_ptr, (int, np.integer)) or isinstance(d_ptr, bool) or int(d_ptr) < 0:
            raise ValueError(f"d_ptr must be a device address, not {d_ptr!r}")
        check(lib().mirt_ctx_update_spheres_device(self._h, int(first), int(count), C.c_void_p(int(d_ptr))))

    def set_spheres(self, spheres) -> None:
        """mirt_ctx_set_spheres: the MIRT_SCENE_HBM scene gets `spheres` (see sphere_records; centre, radius and material_idx are
        read) as its new sphere table -- any count, 0 included -- and a tree built on the device; camera, materials, texels and sky
        stay.  The context is then what set_scene(..., hbm=True, bvh="device") of that scene leaves.  Blocking."""
        ptr, count, keep = sphere_records(spheres)
        _check_range(0, count)
        check(lib().mirt_ctx_set_spheres(self._h, ptr, count))
        del keep

    def set_spheres_device(self, count: int, d_ptr: int) -> None:
        """mirt_ctx_set_spheres_device: the same from `count` 32-byte MirtSphere records in memory of this context's device at
        address `d_ptr` (e.g. a torch tensor's data_ptr(); what was queued to produce them is waited for)."""
        _check_range(0, count)
        if not isinstance(d_ptr, (int, np.integer)) or isinstance(d_ptr, bool) or int(d_ptr) < 0:
            raise ValueError(f"d_ptr must be a device address, not {d_ptr!r}")
        check(lib().mirt_ctx_set_spheres_device(self._h, C.c_void_p(int(d_ptr)) if int(count) else None, int(count)))

    # ---- ray queries against the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
    def trace_rays(self, rays, flags: int = 0, sort: bool = False, lds: bool = False) -> np.ndarray:
        """mirt_ctx_trace_rays: the flat scan's answer for every ray, by the renderer's own arithmetic -> a RAY_HIT_DTYPE array, one
        record per ray in the caller's order; `sphere` == MIRT_RAY_MISS (and everything else 0) for a miss.  `rays`: see ray_records
        (make_rays builds them); flags: MIRT_RAYS_FLAT / _ANY_HIT / _COUNT / _SORT; sort=True sets MIRT_RAYS_SORT: the batch is traced
        in an order derived on the device, the records are the same.  Needs a scene set with hbm=True, or lds=True (MIRT_QUERY_LDS):
        then a scene that lives in LDS answers too, with the same records -- through its uniform grid, or with MIRT_RAYS_FLAT through
        its flat tables; `sort` is then ignored, and an HBM scene ignores `lds`.  Blocking."""
        recs = ray_records(rays)
        flags = _check_rays_flags(flags, sort, lds)
        hits = np.zeros(len(recs), RAY_HIT_DTYPE)
        check(lib().mirt_ctx_trace_rays(self._h, C.c_void_p(recs.ctypes.data) if len(recs) else None, len(recs), flags,
                                        C.c_void_p(hits.ctypes.data) if len(recs) else None))
        self._note_sorted(flags & _abi.MIRT_RAYS_SORT, len(recs))
        return hits

    def trace_rays_device(self, d_rays: int, n: int, d_hits: int, flags: int = 0, stream: Optional[int] = None, sort: bool = False, lds: bool = False) -> None:
        """mirt_ctx_trace_rays_device: `n` 32-byte MirtRay records at device address `d_rays` -> `n` MirtRayHit records at `d_hits`
        (e.g. torch tensors' data_ptr()), asynchronously on `stream` (see _stream_arg); no host synchronisation (sort=True: unless the
        context's sort scratch must grow; sorted launches of one context are kept in order by the caller).  lds: as in trace_rays."""
        _check_range(0, n)
        flags = _check_rays_flags(flags, sort, lds)
        if int(n):
            d_rays, d_hits = _check_address("d_rays", d_rays), _check_address("d_hits", d_hits)
        check(lib().mirt_ctx_trace_rays_device(self._h, C.c_void_p(d_rays) if int(n) else None, int(n), flags,
                                               C.c_void_p(d_hits) if int(n) else None, _stream_arg(stream)))
        self._note_sorted(flags & _abi.MIRT_RAYS_SORT, int(n))

    def trace_stats(self) -> dict:
        """mirt_ctx_trace_stats: waits for the last trace call -> {"kernel_ms", "rays", "sphere_tests", "roots", "hits", "nodes",
        "wave_nodes"}; the counters are 0 unless that call had MIRT_RAYS_COUNT."""
        st = _abi.MirtRayStats()
        check(lib().mirt_ctx_trace_stats(self._h, C.byref(st)))
        return st.as_dict()

    def _note_sorted(self, sort, n: int) -> None:
        if sort and n and getattr(self, "_scene_hbm", True):       # (a scene in LDS, reached with lds=True, ignores the hint: no sorted launch)
            self._sorted_n = n

    def trace_order(self) -> np.ndarray:
        """mirt_ctx_trace_order_read: the permutation of the last sorted launch (trace_rays / trace_radiance with sort=True) on this
        context -> uint32 [n_rays]; order[k] = the caller's index of the ray that ran in slot k, ascending (ray_sort_codes, index).
        Blocking; MirtError before the first sorted launch."""
        order = np.zeros(max(getattr(self, "_sorted_n", 0), 1), np.uint32)
        check(lib().mirt_ctx_trace_order_read(self._h, C.c_void_p(order.ctypes.data), order.size))
        return order[:getattr(self, "_sorted_n", 0)]

    # ---- path-traced radiance for a caller's rays against the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
    def trace_radiance(self, rays, spp: int, *, sample_begin: int = 0, num_bounces: int = 8, seed: int = 0, flat: bool = False,
                       hosek: bool = False, into: Optional[np.ndarray] = None, sort: bool = False, pool: bool = False, lds: bool = False) -> np.ndarray:
        """mirt_ctx_trace_radiance: `spp` samples of the path tracer for every ray -> a RADIANCE_DTYPE array {"sum" [3] in 2^-20 units,
        "samples"}, one record per ray in the caller's order (radiance_mean gives the means).  A sample is the renderer's from its
        primary ray on: samples sample_begin .. sample_begin + spp - 1 of the RNG stream a pixel of index `stream` has under `seed`.
        `rays`: see radiance_ray_records (make_radiance_rays builds them).  flat=True: the flat scan instead of the tree; hosek=True:
        the scene's Hosek sky.  into: a RADIANCE_DTYPE array [n] to ADD to (MIRT_RADIANCE_ACCUMULATE), changed in place and
        returned -- a progressive probe passes sample_begin = the samples it holds.  sort=True (MIRT_RADIANCE_SORT): the batch runs in
        an order derived on the device, for batches that are not in a coherent order; the records are the same.  pool=True (MIRT_RADIANCE_POOL): a hint to run the
        pooled schedule, which deals the samples of 16 rays to a wave's lanes (Context.last_kernel tells whether it ran); the records are
        the same.  Needs a scene set with hbm=True, or lds=True (MIRT_QUERY_LDS): then a scene that lives in LDS answers too, with the
        same records (its grid, or with flat=True its flat tables; `sort` and `pool` are then ignored); an HBM scene ignores `lds`.
        Blocking."""
        recs = radiance_ray_records(rays)
        params = _radiance_params(spp, sample_begin, num_bounces, seed, flat, hosek, into is not None, sort, pool, lds)
        if into is None:
            out = np.zeros(len(recs), RADIANCE_DTYPE)
        else:
            if not isinstance(into, np.ndarray) or into.dtype != RADIANCE_DTYPE or into.shape != (len(recs),) or not into.flags.c_contiguous or not into.flags.writeable:
                raise ValueError("into must be a writable contiguous RADIANCE_DTYPE array with one record per ray")
            out = into
        check(lib().mirt_ctx_trace_radiance(self._h, C.c_void_p(recs.ctypes.data) if len(recs) else None, len(recs), C.byref(params),
                                            C.c_void_p(out.ctypes.data) if len(recs) else None))
        self._note_sorted(sort, len(recs))
        return out

    def trace_radiance_device(self, d_rays: int, n: int, d_out: int, spp: int, *, sample_begin: int = 0, num_bounces: int = 8, seed: int = 0,
                              flat: bool = False, hosek: bool = False, accumulate: bool = False, stream: Optional[int] = None,
                              sort: bool = False, pool: bool = False, lds: bool = False) -> None:
        """mirt_ctx_trace_radiance_device: `n` 32-byte MirtRadianceRay records at device address `d_rays` -> `n` MirtRadiance records at
        `d_out` (e.g. torch tensors' data_ptr()), one kernel queued on `stream` (see _stream_arg); no host synchronisation.
        accumulate=True adds to the records already at `d_out`.  sort=True: the code kernel and the sort are queued in front of it (sorted
        launches of one context are kept in order by the caller).  pool=True: the pooled schedule (a hint, as in trace_radiance).
        lds: as in trace_radiance."""
        _check_range(0, n)
        params = _radiance_params(spp, sample_begin, num_bounces, seed, flat, hosek, accumulate, sort, pool, lds)
        if int(n):
            d_rays, d_out = _check_address("d_rays", d_rays), _check_address("d_out", d_out)
        check(lib().mirt_ctx_trace_radiance_device(self._h, C.c_void_p(d_rays) if int(n) else None, int(n), C.byref(params),
                                                   C.c_void_p(d_out) if int(n) else None, _stream_arg(stream)))
        self._note_sorted(sort, int(n))

    # ---- first-hit feature frames of the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
    def render_features(self, params: _abi.MirtParams, flat: bool = False, lds: bool = False) -> np.ndarray:
        """mirt_ctx_render_features: what the camera sees first at every pixel of the rows `params` selects -> a FEATURE_DTYPE array
        [rows, width] {"albedo", "t", "normal", "sphere"}; `sphere` == MIRT_RAY_MISS and `t` == 0 where the centre ray leaves the scene.
        params.spp == 0: the centre ray alone; spp >= 1: albedo and normal are means over the renderer's own primary rays of those
        samples.  flat=True runs the flat scan instead of the tree (the comparison build).  Needs a scene set with hbm=True, or
        lds=True (MIRT_QUERY_LDS): then a scene that lives in LDS answers too, with the same records (its grid, or with flat=True its
        flat tables); an HBM scene ignores `lds`.  Blocking."""
        params = _check_params(params)
        if not isinstance(flat, (bool, np.bool_)):
            raise ValueError(f"flat must be a bool, not {flat!r}")
        lds_flag = _lds_flag(lds)
        rows, width = max(params_out_rows(params), 0), int(params.width)
        buf = np.zeros(max(rows * width, 1), FEATURE_DTYPE)              # (never a null pointer: a part may own no row)
        check(lib().mirt_ctx_render_features(self._h, C.byref(params), (_abi.MIRT_FEATURES_FLAT if flat else 0) | lds_flag,
                                             C.c_void_p(buf.ctypes.data), rows * width * FEATURE_DTYPE.itemsize))
        return buf[:rows * width].reshape(rows, width)

    def render_features_device(self, params: _abi.MirtParams, d_ptr: int, nbytes: int, flat: bool = False, stream: Optional[int] = None, lds: bool = False) -> None:
        """mirt_ctx_render_features_device: the same records into `nbytes` of device memory at `d_ptr` (4-byte aligned, e.g. a torch
        tensor's data_ptr()), one kernel queued on `stream` (see _stream_arg); no host synchronisation.  lds: as in render_features."""
        params = _check_params(params)
        if not isinstance(flat, (bool, np.bool_)):
            raise ValueError(f"flat must be a bool, not {flat!r}")
        lds_flag = _lds_flag(lds)
        d_ptr = _check_address("d_ptr", d_ptr)
        if not isinstance(nbytes, (int, np.integer)) or isinstance(nbytes, bool) or int(nbytes) < 0:
            raise ValueError(f"nbytes must be a byte count, not {nbytes!r}")
        check(lib().mirt_ctx_render_features_device(self._h, C.byref(params), (_abi.MIRT_FEATURES_FLAT if flat else 0) | lds_flag, C.c_void_p(d_ptr),
                                                    int(nbytes), _stream_arg(stream)))

    # ---- the a-trous filter over the accumulation or the adaptive records (include/mirt.h) ----
    def denoise(self, params: _abi.MirtParams, denoise: _abi.MirtDenoiseParams, guides: np.ndarray) -> np.ndarray:
        """mirt_ctx_denoise: the filtered frame of the source `denoise` names, guided by `guides` -- a FEATURE_DTYPE array with one record
        per pixel of the band, what render_features returned for the same width, height and rows -> uint8 [rows, width, 4], or float32
        [rows, width, 4] (linear {r, g, b, 1}) with MIRT_DENOISE_OUT_F32.  Reads no scene; sums, records and guides stay as they are.
        Blocking."""
        params, denoise = _check_params(params), _check_denoise(denoise)
        if not isinstance(guides, np.ndarray) or guides.dtype != FEATURE_DTYPE:
            raise ValueError("guides must be a FEATURE_DTYPE array")
        g = np.ascontiguousarray(guides).reshape(-1)
        rows, width = max(params_out_rows(params), 0), int(params.width)
        f32 = bool(denoise.flags & _abi.MIRT_DENOISE_OUT_F32)
        out = np.zeros((max(rows, 1), max(width, 1), 4), np.float32 if f32 else np.uint8)
        check(lib().mirt_ctx_denoise(self._h, C.byref(params), C.byref(denoise), C.c_void_p(g.ctypes.data) if len(g) else None, g.nbytes,
                                     C.c_void_p(out.ctypes.data), rows * width * (16 if f32 else 4)))
        return out[:rows, :width]

    def denoise_device(self, params: _abi.MirtParams, denoise: _abi.MirtDenoiseParams, d_guides: int, guides_nbytes: int, d_out: int, nbytes: int,
                       stream: Optional[int] = None) -> None:
        """mirt_ctx_denoise_device: the same with the guides (`guides_nbytes` at `d_guides`) and the output (`nbytes` at `d_out`) in
        device memory, both 4-byte aligned, queued on `stream` (see _stream_arg); no host synchronisation unless the context's scratch
        must grow."""
        params, denoise = _check_params(params), _check_denoise(denoise)
        d_guides, d_out = _check_address("d_guides", d_guides), _check_address("d_out", d_out)
        for name, v in (("guides_nbytes", guides_nbytes), ("nbytes", nbytes)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or int(v) < 0:
                raise ValueError(f"{name} must be a byte count, not {v!r}")
        check(lib().mirt_ctx_denoise_device(self._h, C.byref(params), C.byref(denoise), C.c_void_p(d_guides), int(guides_nbytes), C.c_void_p(d_out),
                                            int(nbytes), _stream_arg(stream)))

    # ---- temporal reprojection of a denoised frame (include/mirt.h) ----
    def reproject(self, params: _abi.MirtParams, reproject: _abi.MirtReprojectParams, colour: np.ndarray, guides: np.ndarray, prev_colour: np.ndarray,
                  prev_guides: np.ndarray, *, rgba8: bool = False):
        """mirt_ctx_reproject: this frame's `colour` (float32 [rows, width, 4], what denoise wrote with MIRT_DENOISE_OUT_F32) blended
        with the previous frame's result `prev_colour` ({r, g, b, history length}: the result of the previous call, or a denoise
        output) taken to this frame's pixels by the first-hit depth and id of `guides` / `prev_guides` (FEATURE_DTYPE [rows, width],
        taken with reproject.current / reproject.previous) -> float32 [rows, width, 4] = {r, g, b, new history length}; with
        rgba8=True a pair of that and uint8 [rows, width, 4] per params.flags.  Reads no scene and no state of the context.  Blocking."""
        params, reproject = _check_params(params), _check_reproject(reproject)
        if not isinstance(rgba8, (bool, np.bool_)):
            raise ValueError(f"rgba8 must be a bool, not {rgba8!r}")
        named = (("colour", colour, np.float32, (4,)), ("guides", guides, FEATURE_DTYPE, ()), ("prev_colour", prev_colour, np.float32, (4,)),
                 ("prev_guides", prev_guides, FEATURE_DTYPE, ()))
        for name, a, dt, tail in named:
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 2 + len(tail):
                raise ValueError(f"{name} must be a {'float32 [rows, width, 4]' if tail else 'FEATURE_DTYPE [rows, width]'} array")
        rows, width = max(params_out_rows(params), 0), int(params.width)
        planes = []
        for name, a, dt, tail in named:
            if a.shape != (rows, width) + tail:
                raise ValueError(f"{name} has shape {a.shape}, the band is {(rows, width) + tail}")
            planes.append(np.ascontiguousarray(a))
        n = rows * width
        out = np.zeros((max(rows, 1), max(width, 1), 4), np.float32)
        rgba = np.zeros((max(rows, 1), max(width, 1), 4), np.uint8)
        spare = [np.zeros(1, dt) for dt in (np.float32, FEATURE_DTYPE, np.float32, FEATURE_DTYPE)]       # a band without rows: the pointers stay non-null
        f = _abi.MirtReprojectFrames()
        f.colour, f.guides, f.prev_colour, f.prev_guides = (a.ctypes.data if n else s.ctypes.data for a, s in zip(planes, spare))
        f.out, f.out_rgba8, f.pixels = out.ctypes.data, rgba.ctypes.data if rgba8 else None, n
        check(lib().mirt_ctx_reproject(self._h, C.byref(params), C.byref(reproject), C.byref(f)))
        out, rgba = out[:rows, :width], rgba[:rows, :width]
        return (out, rgba) if rgba8 else out

    def reproject_device(self, params: _abi.MirtParams, reproject: _abi.MirtReprojectParams, d_colour: int, d_guides: int, d_prev_colour: int, d_prev_guides: int,
                         d_out: int, pixels: int, *, d_out_rgba8: Optional[int] = None, stream: Optional[int] = None) -> None:
        """mirt_ctx_reproject_device: the same with all planes in device memory (addresses, 4-byte aligned, `pixels` records each; 16
        bytes per colour record, 32 per guide record, 4 per RGBA8 pixel), queued on `stream` (see _stream_arg).  d_out_rgba8=None: no
        RGBA8 plane.  Never synchronises; the caller orders it against the calls that produce its inputs."""
        params, reproject = _check_params(params), _check_reproject(reproject)
        f = _abi.MirtReprojectFrames()
        f.colour, f.guides = _check_address("d_colour", d_colour), _check_address("d_guides", d_guides)
        f.prev_colour, f.prev_guides = _check_address("d_prev_colour", d_prev_colour), _check_address("d_prev_guides", d_prev_guides)
        f.out = _check_address("d_out", d_out)
        f.out_rgba8 = None if d_out_rgba8 is None else _check_address("d_out_rgba8", d_out_rgba8)
        if not isinstance(pixels, (int, np.integer)) or isinstance(pixels, bool) or not 0 <= int(pixels) < 2 ** 64:
            raise ValueError(f"pixels must be a record count, not {pixels!r}")
        f.pixels = int(pixels)
        check(lib().mirt_ctx_reproject_device(self._h, C.byref(params), C.byref(reproject), C.byref(f), _stream_arg(stream)))

    def bvh_refits(self) -> int:
        """mirt_ctx_bvh_refits: successful updates since the scene was set (0 after every set_scene)."""
        return int(lib().mirt_ctx_bvh_refits(self._h))

    def set_camera(self, camera: _abi.MirtGpuCamera) -> None:
        check(lib().mirt_ctx_set_camera(self._h, C.byref(camera)))

    def render(self, params: _abi.MirtParams) -> np.ndarray:
        """Render to host memory -> uint8 [rows, width, 4] (RGBA8, top row first)."""
        rows = params_out_rows(params)
        out = np.empty((max(rows, 0), params.width, 4), dtype=np.uint8)
        check(lib().mirt_ctx_render(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def render_device(self, params: _abi.MirtParams, d_ptr: int, nbytes: int, stream: Optional[int] = None) -> None:
        """Render asynchronously into device memory (e.g. a torch uint8 CUDA tensor's data_ptr()) on `stream`
        (see _stream_arg: None = the context's stream, 0 = the default stream, else a hipStream_t handle)."""
        check(lib().mirt_ctx_render_device(self._h, C.byref(params), C.c_void_p(d_ptr), nbytes, _stream_arg(stream)))

    def deinterleave_device(self, params: _abi.MirtParams, d_parts: int, part_stride: int, d_out: int,
                            out_nbytes: int, stream: Optional[int] = None) -> None:
        check(lib().mirt_ctx_deinterleave_device(self._h, C.byref(params), C.c_void_p(d_parts), part_stride,
                                                 C.c_void_p(d_out), out_nbytes, _stream_arg(stream)))

    # ---- progressive accumulation (RenderProgress::next_frame + the shader's image buffer) ----
    def accum_reset(self, params: _abi.MirtParams) -> None:
        check(lib().mirt_ctx_accum_reset(self._h, C.byref(params)))

    def accum_add(self, params: _abi.MirtParams, stream: Optional[int] = None) -> None:
        check(lib().mirt_ctx_accum_add(self._h, C.byref(params), _stream_arg(stream)))

    def accum_samples(self) -> int:
        return int(lib().mirt_ctx_accum_samples(self._h))

    def accum_resolve(self, params: _abi.MirtParams) -> np.ndarray:
        out = np.empty((params_out_rows(params), params.width, 4), dtype=np.uint8)
        check(lib().mirt_ctx_accum_resolve(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def accum_read(self, params: _abi.MirtParams) -> np.ndarray:
        out = np.empty((params_out_rows(params), params.width, 3), dtype=np.uint64)
        check(lib().mirt_ctx_accum_read(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def accum_frame_device(self, params: _abi.MirtParams, d_out: int, stream: Optional[int] = None, nbytes: Optional[int] = None) -> None:
        """mirt_ctx_accum_frame_device: ONE progressive frame in one launch -- `params.spp` further samples added to the sums and the
        resolve of the updated sums written to device memory at address `d_out` (rows x width x 4 bytes unless `nbytes` says more),
        asynchronously on `stream` (see _stream_arg).  params.spp == 0: the mean of what is there, nothing added."""
        if nbytes is None:
            nbytes = params_out_rows(params) * params.width * 4
        check(lib().mirt_ctx_accum_frame_device(self._h, C.byref(params), C.c_void_p(d_out), nbytes, _stream_arg(stream)))

    def accum_frame(self, params: _abi.MirtParams) -> np.ndarray:
        """The same frame to host memory (mirt_ctx_accum_frame; blocking) -> uint8 [rows, width, 4]."""
        out = np.empty((params_out_rows(params), params.width, 4), dtype=np.uint8)
        check(lib().mirt_ctx_accum_frame(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ---- adaptive sampling for progressive frames of the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
    def adapt_reset(self, params: _abi.MirtParams) -> None:
        """mirt_ctx_adapt_reset: one cleared 64-byte record per pixel of the rows `params` selects (a buffer apart from accum_*)."""
        check(lib().mirt_ctx_adapt_reset(self._h, C.byref(_check_params(params))))

    def adapt_step(self, params: _abi.MirtParams, adapt: _abi.MirtAdaptParams, stream: Optional[int] = None) -> None:
        """mirt_ctx_adapt_step_device: one adaptive step on `stream` (see _stream_arg), no host synchronisation -- the rule for every
        record, the active pixels listed in ascending order, then exactly params.spp (even) further samples for every listed pixel."""
        if not isinstance(adapt, _abi.MirtAdaptParams):
            raise ValueError(f"adapt must be a MirtAdaptParams (make_adapt_params builds one), not {type(adapt).__name__}")
        check(lib().mirt_ctx_adapt_step_device(self._h, C.byref(_check_params(params)), C.byref(adapt), _stream_arg(stream)))

    def adapt_run(self, params: _abi.MirtParams, adapt: _abi.MirtAdaptParams, run: _abi.MirtAdaptRun, stream: Optional[int] = None) -> None:
        """mirt_ctx_adapt_run_device: run.max_steps adaptive steps queued on `stream` (see _stream_arg) by ONE call, no host
        synchronisation -- every step selects as adapt_step does and its sample count is chosen on the device from the list it has
        just built (make_adapt_run); steps behind an empty one change nothing.  adapt_run_log() has the counts and step sizes."""
        if not isinstance(adapt, _abi.MirtAdaptParams):
            raise ValueError(f"adapt must be a MirtAdaptParams (make_adapt_params builds one), not {type(adapt).__name__}")
        if not isinstance(run, _abi.MirtAdaptRun):
            raise ValueError(f"run must be a MirtAdaptRun (make_adapt_run builds one), not {type(run).__name__}")
        check(lib().mirt_ctx_adapt_run_device(self._h, C.byref(_check_params(params)), C.byref(adapt), C.byref(run), _stream_arg(stream)))

    def adapt_run_log(self) -> np.ndarray:
        """mirt_ctx_adapt_run_read: the last run's log -> uint32 [max_steps, 2], {count, spp} per step; blocking."""
        n = C.c_uint32()
        buf = np.zeros((_abi.MIRT_ADAPT_RUN_MAX_STEPS, 2), np.uint32)
        check(lib().mirt_ctx_adapt_run_read(self._h, C.c_void_p(buf.ctypes.data), len(buf), C.byref(n)))
        return buf[:n.value].copy()

    def adapt_resolve(self, params: _abi.MirtParams) -> np.ndarray:
        """mirt_ctx_adapt_resolve: every pixel's mean over ITS samples, tone curves per params.flags -> uint8 [rows, width, 4]; blocking."""
        params = _check_params(params)
        out = np.empty((max(params_out_rows(params), 0), params.width, 4), dtype=np.uint8)
        check(lib().mirt_ctx_adapt_resolve(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def adapt_resolve_device(self, params: _abi.MirtParams, d_out: int, stream: Optional[int] = None, nbytes: Optional[int] = None) -> None:
        """mirt_ctx_adapt_resolve_device: the same into device memory at `d_out` (rows x width x 4 bytes unless `nbytes` says more)
        on `stream`; no host synchronisation."""
        params = _check_params(params)
        if nbytes is None:
            nbytes = params_out_rows(params) * params.width * 4
        check(lib().mirt_ctx_adapt_resolve_device(self._h, C.byref(params), C.c_void_p(_check_address("d_out", d_out)), int(nbytes), _stream_arg(stream)))

    def adapt_read(self) -> np.ndarray:
        """mirt_ctx_adapt_read: the records -> an ADAPT_PIXEL_DTYPE array [pixels], the pixels of the band row-major; blocking."""
        out = np.zeros(max(self.adapt_stats()["pixels"], 1), ADAPT_PIXEL_DTYPE)
        check(lib().mirt_ctx_adapt_read(self._h, C.c_void_p(out.ctypes.data), out.size))
        return out[:self.adapt_stats()["pixels"]]

    def adapt_write(self, records: np.ndarray) -> None:
        """mirt_ctx_adapt_write: replaces the records (an ADAPT_PIXEL_DTYPE array with one record per pixel of the buffer); blocking."""
        if not isinstance(records, np.ndarray) or records.dtype != ADAPT_PIXEL_DTYPE:
            raise ValueError("records must be an ADAPT_PIXEL_DTYPE array")
        recs = np.ascontiguousarray(records).reshape(-1)
        check(lib().mirt_ctx_adapt_write(self._h, C.c_void_p(recs.ctypes.data) if len(recs) else None, len(recs)))

    def adapt_list(self) -> np.ndarray:
        """mirt_ctx_adapt_list_read: the pixels the last step sampled -> uint32 [count], ascending places in the band; blocking."""
        n = C.c_uint32()
        buf = np.zeros(max(self.adapt_stats()["pixels"], 1), np.uint32)
        check(lib().mirt_ctx_adapt_list_read(self._h, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)))
        return buf[:n.value].copy()

    def adapt_stats(self) -> dict:
        """mirt_ctx_adapt_stats: waits for the last step -> {"pixels", "total_samples", "active", "steps", "kernel_ms"}."""
        st = _abi.MirtAdaptStats()
        check(lib().mirt_ctx_adapt_stats(self._h, C.byref(st)))
        return st.as_dict()

    def selftest_math(self) -> tuple:
        """(sqrt mismatches, reciprocal mismatches) of the fast sequences vs IEEE over all 2^32 floats."""
        out = (C.c_uint64 * 2)()
        check(lib().mirt_ctx_selftest_math(self._h, out))
        return int(out[0]), int(out[1])

    def selftest_checker_sign(self) -> tuple:
        """(decided, parity mismatches, zeros) of the checkerboard's fast sign path, axis by axis over all 2^32 floats."""
        out = (C.c_uint64 * 3)()
        check(lib().mirt_ctx_selftest_checker_sign(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def last_kernel(self) -> str:
        """Name of the render kernel the last render call launched (as rocprofv3 traces spell it)."""
        s = lib().mirt_ctx_last_kernel(self._h)
        return s.decode() if s else ""

    def synchronize(self) -> None:
        check(lib().mirt_ctx_synchronize(self._h))

    def frame_stream(self, index: int) -> int:
        """hipStream_t handle (an int for the `stream` arguments here) of the context's frame stream 0 or 1: two streams on different
        hardware queues for hosts that keep two frames in flight (mirt_ctx_frame_stream)."""
        h = C.c_void_p()
        check(lib().mirt_ctx_frame_stream(self._h, index, C.byref(h)))
        return int(h.value)

    def set_timing(self, enabled: bool) -> None:
        """Kernel timing on (default: every launch carries an event pair, `stats()` reports kernel times) or off (launches carry no
        event unless the context needs one: the reference's interactive frames queue back to back 30 % faster)."""
        check(lib().mirt_ctx_set_timing(self._h, 1 if enabled else 0))

    def stats(self) -> dict:
        st = _abi.MirtStats()
        check(lib().mirt_ctx_get_stats(self._h, C.byref(st)))
        return st.as_dict()
