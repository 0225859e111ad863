"""Host-side mirror of the reference's interface for the per-pixel path: the names, argument
meaning and error behaviour of `src/raytracer/{mod,layer,texture,angle}.rs` and the default pose of
`src/fly_camera.rs`, with `Layer::set_data` implemented as ONE call into the HIP library.

Nothing here computes pixels: `Layer.set_data` / `Raytracer.render` go through the C ABI
(include/mirt.h) to the gfx950 kernels, and fail if libmirt.so or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from ._lib import MirtError, check, lib
from .context import Context, FEATURE_DTYPE, SceneData, make_params, make_rays, radiance_mean, set_scene_any_size
from .node import Node

f32 = np.float32


def _v3(v) -> np.ndarray:
    a = np.asarray(v, dtype=np.float32).reshape(3)
    return a


# ------------------------------------------------------------------------------------------------
# Angle — src/raytracer/angle.rs:1-50
# ------------------------------------------------------------------------------------------------

@dataclass(frozen=True, order=True)
class Angle:
    _radians: float

    @staticmethod
    def degrees(degrees: float) -> "Angle":          # angle.rs:8-12
        return Angle(float(lib().mirt_degrees_to_radians(C.c_float(degrees))))

    @staticmethod
    def radians(radians: float) -> "Angle":          # angle.rs:15-17
        return Angle(float(f32(radians)))

    def as_degrees(self) -> float:                   # angle.rs:20-22
        return float(lib().mirt_radians_to_degrees(C.c_float(self._radians)))

    def as_radians(self) -> float:                   # angle.rs:25-27
        return self._radians

    def clamp(self, lo: "Angle", hi: "Angle") -> "Angle":   # angle.rs:29-39
        r = self._radians
        if r < lo._radians:
            r = lo._radians
        if r > hi._radians:
            r = hi._radians
        return Angle(r)

    def __add__(self, rhs: "Angle") -> "Angle":      # angle.rs:42-50
        return Angle(float(f32(self._radians) + f32(rhs._radians)))


# ------------------------------------------------------------------------------------------------
# Camera / GpuCamera / params — src/raytracer/mod.rs:440-541, 597-613, 681-755
# ------------------------------------------------------------------------------------------------

@dataclass
class Camera:
    eye_pos: np.ndarray
    eye_dir: np.ndarray
    up: np.ndarray
    vfov: Angle
    aperture: float
    focus_distance: float

    def to_c(self) -> _abi.MirtCamera:
        c = _abi.MirtCamera()
        c.eye_pos[:] = _v3(self.eye_pos).tolist()
        c.eye_dir[:] = _v3(self.eye_dir).tolist()
        c.up[:] = _v3(self.up).tolist()
        c.vfov_radians = self.vfov.as_radians()
        c.aperture = self.aperture
        c.focus_distance = self.focus_distance
        return c

    @staticmethod
    def from_c(c: _abi.MirtCamera) -> "Camera":
        return Camera(np.array(c.eye_pos[:], dtype=f32), np.array(c.eye_dir[:], dtype=f32),
                      np.array(c.up[:], dtype=f32), Angle(float(c.vfov_radians)), float(c.aperture),
                      float(c.focus_distance))


class GpuCamera:
    """`GpuCamera::new(&camera, viewport_size)` mod.rs:700-741 (host arithmetic inside libmirt)."""

    def __init__(self, c: _abi.MirtGpuCamera):
        self.c = c

    @staticmethod
    def new(camera: Camera, viewport_size: Tuple[int, int]) -> "GpuCamera":
        out = _abi.MirtGpuCamera()
        cam = camera.to_c()
        check(lib().mirt_camera_new(C.byref(cam), int(viewport_size[0]), int(viewport_size[1]), C.byref(out)))
        return GpuCamera(out)

    def as_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self.c), dtype=np.float32).copy()


@dataclass
class SamplingParams:                                  # mod.rs:597-613
    max_samples_per_pixel: int = 128
    num_samples_per_pixel: int = 2
    num_bounces: int = 8

    def to_c(self) -> _abi.MirtSamplingParams:
        return _abi.MirtSamplingParams(self.max_samples_per_pixel, self.num_samples_per_pixel, self.num_bounces)


@dataclass
class SkyParams:                                       # mod.rs:543-565 (defaults)
    azimuth_degrees: float = 0.0
    zenith_degrees: float = 85.0
    turbidity: float = 4.0
    albedo: Tuple[float, float, float] = (1.0, 1.0, 1.0)


class RenderParamsValidationError(ValueError):
    """mod.rs:396-411; `.kind` is the Rust variant name."""
    KINDS = {
        _abi.MIRT_ERR_MAX_SAMPLES_MULTIPLE: "MaxSampleCountNotMultiple",
        _abi.MIRT_ERR_VIEWPORT_SIZE: "ViewportSize",
        _abi.MIRT_ERR_VFOV_RANGE: "VfovOutOfRange",
        _abi.MIRT_ERR_APERTURE_RANGE: "ApertureOutOfRange",
        _abi.MIRT_ERR_FOCUS_DISTANCE: "FocusDistanceOutOfRange",
        _abi.MIRT_ERR_SKY: "HwSkyModelValidationError",
        _abi.MIRT_ERR_SPP_ZERO: "NumSamplesZero",
    }

    def __init__(self, status: int, message: str):
        self.status = status
        self.kind = self.KINDS.get(status, "Unknown")
        super().__init__(message)


@dataclass
class RenderParams:                                    # mod.rs:442-447
    camera: Camera
    sky: SkyParams = field(default_factory=SkyParams)
    sampling: SamplingParams = field(default_factory=SamplingParams)
    viewport_size: Tuple[int, int] = (800, 600)

    def validate(self) -> None:                        # mod.rs:450-484
        cam, smp = self.camera.to_c(), self.sampling.to_c()
        rc = lib().mirt_validate_render_params(C.byref(cam), C.byref(smp), int(self.viewport_size[0]),
                                               int(self.viewport_size[1]))
        if rc != _abi.MIRT_OK:
            raise RenderParamsValidationError(rc, lib().mirt_last_error().decode())


# ------------------------------------------------------------------------------------------------
# FlyCameraController — default pose + camera_orientation, src/fly_camera.rs:24-64, 227-241
# ------------------------------------------------------------------------------------------------

@dataclass
class FlyCameraController:
    position: np.ndarray
    yaw: Angle
    pitch: Angle
    vfov_degrees: float
    aperture: float
    focus_distance: float

    @staticmethod
    def default() -> "FlyCameraController":           # fly_camera.rs:24-50
        look_from = np.array([-10.0, 2.0, -4.0], dtype=f32)
        look_at = np.array([0.0, 1.0, 0.0], dtype=f32)
        d = (look_at - look_from).astype(f32)
        # glm::magnitude = sqrt((d0*d0 + d1*d1) + d2*d2) in f32
        focus = float(np.sqrt(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]), dtype=f32))
        return FlyCameraController(look_from, Angle.degrees(25.0), Angle.degrees(-10.0), 30.0, 0.8, focus)

    def renderer_camera(self) -> Camera:              # fly_camera.rs:52-64
        out = _abi.MirtCamera()
        pos = (C.c_float * 3)(*_v3(self.position).tolist())
        check(lib().mirt_camera_from_fly_pose(pos, self.yaw.as_radians(), self.pitch.as_radians(),
                                              self.vfov_degrees, self.aperture, self.focus_distance, C.byref(out)))
        return Camera.from_c(out)


# ------------------------------------------------------------------------------------------------
# Scene model — mod.rs:413-438, 757-886; texture.rs:9-78
# ------------------------------------------------------------------------------------------------

class Sphere:
    """`Sphere::new(center, radius, material_idx)` mod.rs:423-431 -> 32-byte wire struct."""

    def __init__(self, center, radius: float, material_idx: int):
        self.center = _v3(center)
        self.radius = float(f32(radius))
        self.material_idx = int(material_idx)

    @staticmethod
    def new(center, radius: float, material_idx: int) -> "Sphere":
        return Sphere(center, radius, material_idx)

    def to_c(self) -> _abi.MirtSphere:
        s = _abi.MirtSphere()
        s.center[:] = [float(self.center[0]), float(self.center[1]), float(self.center[2]), 0.0]
        s.radius = self.radius
        s.material_idx = self.material_idx
        return s


class Texture:
    """texture.rs:9-78: dimensions + `Vec<[f32;3]>` (row-major, top row first)."""

    def __init__(self, dimensions: Tuple[int, int], data: np.ndarray):
        self._dimensions = (int(dimensions[0]), int(dimensions[1]))
        self._data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1, 3)
        assert self._data.shape[0] == self._dimensions[0] * self._dimensions[1]

    @staticmethod
    def new_from_rgb8(rgb8: np.ndarray) -> "Texture":
        """[h][w][3] uint8 -> texels `inv_255 * (p as f32)` exactly as texture.rs:30-41."""
        rgb8 = np.asarray(rgb8, dtype=np.uint8)
        h, w, _ = rgb8.shape
        inv_255 = f32(1.0) / f32(255.0)
        data = (inv_255 * rgb8.astype(np.float32)).astype(np.float32)
        return Texture((w, h), data)

    @staticmethod
    def new_from_image(path: str) -> "Texture":       # texture.rs:21-46
        """Decode an image file.  `.npz` (key `rgb8`) and `.npy` hold already-decoded RGB8 texels; anything else is read
        as a JPEG (the reference passes `ImageFormat::Jpeg`, texture.rs:27-28) and decoded by the library's own decoder
        (csrc/mirt_jpeg.cpp: bit-identical to libjpeg-turbo; DECODER-UNPINNED against the `image` crate's jpeg-decoder,
        +-1 LSB in some texels is possible and nothing in the reference pins either)."""
        p = Path(path)
        if not p.exists():
            raise FileNotFoundError(path)             # TextureError::FileIoError
        if p.suffix == ".npz":
            return Texture.new_from_rgb8(np.load(p)["rgb8"])
        if p.suffix == ".npy":
            return Texture.new_from_rgb8(np.load(p))
        return Texture.new_from_jpeg_bytes(p.read_bytes())

    @staticmethod
    def new_from_jpeg_bytes(data: bytes) -> "Texture":
        """JPEG bytes -> RGB8 (mirt_jpeg_decode_rgb8) -> `inv_255 * (p as f32)` texels (mirt_rgb8_to_texels)."""
        rgb = decode_jpeg(data)
        h, w, _ = rgb.shape
        texels = np.empty((h * w, 3), dtype=np.float32)
        check(lib().mirt_rgb8_to_texels(rgb.ctypes.data_as(C.c_void_p), h * w, texels.ctypes.data_as(C.c_void_p)))
        return Texture((w, h), texels.reshape(h, w, 3))

    @staticmethod
    def new_from_color(color) -> "Texture":           # texture.rs:48-54
        return Texture((1, 1), _v3(color).reshape(1, 3))

    def as_slice(self) -> np.ndarray:
        return self._data

    def dimensions(self) -> Tuple[int, int]:
        return self._dimensions


class Material:
    """`enum Material` mod.rs:433-438."""

    @dataclass
    class Lambertian:
        albedo: Texture

    @dataclass
    class Metal:
        albedo: Texture
        fuzz: float

    @dataclass
    class Dielectric:
        refraction_index: float

    @dataclass
    class Checkerboard:
        even: Texture
        odd: Texture


class TextureDescriptor:
    @staticmethod
    def empty() -> _abi.MirtTextureDescriptor:        # mod.rs:878-886
        return _abi.MirtTextureDescriptor(0, 0, 0xFFFFFFFF)


class GpuMaterial:
    """mod.rs:767-830: flatten one Material into the 32-byte record + append its texels."""

    @staticmethod
    def _append(texture: Texture, global_texture_data: List[np.ndarray]) -> _abi.MirtTextureDescriptor:
        w, h = texture.dimensions()
        offset = sum(a.shape[0] for a in global_texture_data)
        global_texture_data.append(texture.as_slice())
        return _abi.MirtTextureDescriptor(w, h, offset)

    @staticmethod
    def lambertian(albedo: Texture, gtd: List[np.ndarray]) -> _abi.MirtMaterial:
        return _abi.MirtMaterial(0, GpuMaterial._append(albedo, gtd), TextureDescriptor.empty(), 0.0)

    @staticmethod
    def metal(albedo: Texture, fuzz: float, gtd: List[np.ndarray]) -> _abi.MirtMaterial:
        return _abi.MirtMaterial(1, GpuMaterial._append(albedo, gtd), TextureDescriptor.empty(), float(f32(fuzz)))

    @staticmethod
    def dielectric(refraction_index: float) -> _abi.MirtMaterial:
        return _abi.MirtMaterial(2, TextureDescriptor.empty(), TextureDescriptor.empty(), float(f32(refraction_index)))

    @staticmethod
    def checkerboard(even: Texture, odd: Texture, gtd: List[np.ndarray]) -> _abi.MirtMaterial:
        d1 = GpuMaterial._append(even, gtd)
        d2 = GpuMaterial._append(odd, gtd)
        return _abi.MirtMaterial(3, d1, d2, 0.0)


@dataclass
class Scene:                                           # mod.rs:413-416
    spheres: List[Sphere]
    materials: List[object]


def flatten_materials(materials: Sequence[object]) -> Tuple[List[_abi.MirtMaterial], np.ndarray]:
    """`Layer::set_global_data` layer.rs:125-148 (and the identical loop of Raytracer::new,
    mod.rs:160-183).  NOTE the reference's argument-order quirk: the call sites pass (odd, even)
    into a (even, odd) signature, so desc1 is the ODD colour (layer.rs:139-141 vs mod.rs:802-813)."""
    gtd: List[np.ndarray] = []
    out: List[_abi.MirtMaterial] = []
    for m in materials:
        if isinstance(m, Material.Lambertian):
            out.append(GpuMaterial.lambertian(m.albedo, gtd))
        elif isinstance(m, Material.Metal):
            out.append(GpuMaterial.metal(m.albedo, m.fuzz, gtd))
        elif isinstance(m, Material.Dielectric):
            out.append(GpuMaterial.dielectric(m.refraction_index))
        elif isinstance(m, Material.Checkerboard):
            out.append(GpuMaterial.checkerboard(m.odd, m.even, gtd))
        else:
            raise TypeError(f"not a Material: {m!r}")
    texels = np.concatenate(gtd, axis=0) if gtd else np.zeros((0, 3), dtype=np.float32)
    return out, texels


_ASSET_FIXTURES = {
    "assets/moon.jpeg": "moon_1024x512_rgb8.npz",
    "assets/earthmap.jpeg": "earthmap_1024x512_rgb8.npz",
}


def _moved(held: Sequence[Sphere], first, spheres: Sequence[Sphere]) -> Tuple[int, List[Sphere]]:
    """move_spheres: (first as an int, the new spheres first .. first + len(spheres)) -- centre and radius from `spheres`, the
    material they had."""
    spheres = list(spheres)
    if not isinstance(first, (int, np.integer)) or isinstance(first, bool) or first < 0 or int(first) + len(spheres) > len(held):
        raise ValueError(f"spheres [{first}, {first}+{len(spheres)}) of a scene of {len(held)}")
    if not all(isinstance(s, Sphere) for s in spheres):
        raise ValueError("spheres must be Sphere objects")
    first = int(first)
    return first, [Sphere(s.center, s.radius, held[first + i].material_idx) for i, s in enumerate(spheres)]


def _spliced(held: Sequence[Sphere], first: int, moved: Sequence[Sphere]) -> List[Sphere]:
    out = list(held)
    out[first:first + len(moved)] = moved
    return out


def _move_resident(owner, target, first: int, moved: Sequence[Sphere], scene_data) -> None:
    """The device side of move_spheres of `owner` (a Layer or a Raytracer) on `target` (its Context or Node): an HBM scene is updated
    in place, any other is set again from `scene_data()` (the moved scene).  `owner._hbm` says which the target holds afterwards; a
    failure other than a refused argument may leave the target without a scene, so the owner's next move sets one."""
    if not owner._hbm:
        owner._hbm = set_scene_any_size(target, scene_data())
        return
    try:
        target.update_spheres(first, moved)
    except MirtError as e:
        if e.status not in (_abi.MIRT_ERR_BAD_ROWS, _abi.MIRT_ERR_NULL_POINTER):
            owner._hbm = False
        raise


def _world(spheres: Sequence[Sphere]) -> List[Sphere]:
    """set_world: the new world as a list of Sphere."""
    spheres = list(spheres)
    if not all(isinstance(s, Sphere) for s in spheres):
        raise ValueError("spheres must be Sphere objects")
    return spheres


def _set_world_resident(owner, target, world: Sequence[Sphere], scene_data) -> None:
    """The device side of set_world of `owner` (a Layer or a Raytracer) on `target` (its Context or Node): an HBM scene gets the new
    sphere table in place (its materials and texels stay resident, the tree is built on the device), any other is set again from
    `scene_data()` (the new scene).  `owner._hbm` as in _move_resident."""
    if not owner._hbm:
        owner._hbm = set_scene_any_size(target, scene_data())
        return
    try:
        target.set_spheres(world)
    except MirtError as e:
        if e.status not in (_abi.MIRT_ERR_SCENE_TOO_LARGE, _abi.MIRT_ERR_NULL_POINTER):
            owner._hbm = False
        raise


def pixel_ray(camera: _abi.MirtGpuCamera, width: int, height: int, x: int, y: int) -> Tuple[np.ndarray, np.ndarray]:
    """The pinhole ray through the CENTRE of pixel (x, y), row 0 on top: `cameraMakeRay` (wgsl:345-362) with a zero lens at
    u = (x + 0.5) / width, v = 1 - (y + 0.5) / height, in float32 on the host -> (origin [3], direction [3], not normalised)."""
    if not (0 <= int(x) < int(width) and 0 <= int(y) < int(height)):
        raise ValueError(f"pixel ({x}, {y}) lies outside the {width} x {height} viewport")
    u = f32(f32(x) + f32(0.5)) / f32(width)
    v = f32(1.0) - f32(f32(y) + f32(0.5)) / f32(height)
    eye, hor, ver, llc = (np.asarray(a[:3], f32) for a in (camera.eye, camera.horizontal, camera.vertical, camera.lower_left_corner))
    d = (llc.astype(np.float64) + np.float64(u) * hor + np.float64(v) * ver).astype(f32) - eye
    return eye, d.astype(f32)


def pixel_project(camera: _abi.MirtGpuCamera, width: int, height: int, point) -> Tuple[float, float, float]:
    """Where `point` falls in the viewport: (fx, fy, s) with pixel centres at integers and row 0 on top, and s the parameter of the
    point along the centre ray of that position (s > 0: in front of the camera) -- mirt_camera_project, the rule mirt_ctx_reproject
    takes a first hit to the previous frame with.  pixel_project(c, w, h, origin + t * direction) of pixel_ray(c, w, h, x, y) is
    (x, y, t) up to float32 rounding."""
    from .context import camera_project
    fx, fy, s = camera_project(camera, width, height, point)
    return float(fx), float(fy), float(s)


def _query_target(owner, scene_data, lds):
    """The context a query of Layer / Raytracer runs on (member 0's on a node).  lds=False: the query needs the world in device memory,
    so a resident LDS scene -- or none yet -- is set again as a MIRT_SCENE_HBM scene first (owner._hbm is True afterwards).  lds=True
    (MIRT_QUERY_LDS): whatever is resident stays where it is -- a scene held in LDS answers from there, and later renders keep their
    LDS builds --; with nothing resident yet the library answers MIRT_ERR_NO_SCENE."""
    if not isinstance(lds, (bool, np.bool_)):
        raise ValueError(f"lds must be a bool, not {lds!r}")
    target = owner._pick_target()
    if not owner._hbm and not lds:
        target.set_scene(scene_data(), hbm=True)
        owner._hbm = True
    return target.context(0) if hasattr(target, "context") else target


def _pick(owner, x: int, y: int, width: int, height: int, camera: _abi.MirtGpuCamera, scene_data, lds: bool = False) -> Optional[dict]:
    """Layer.pick / Raytracer.pick: the sphere under pixel (x, y) by Context.trace_rays with t_max = 1000 (what a path of the renderer
    would hit first).  Ray queries need the world in device memory: a resident LDS scene -- or none yet -- is set again as a
    MIRT_SCENE_HBM scene first (the images do not change; owner._hbm is True afterwards) unless lds=True (_query_target).  On a node
    the query runs on member 0's context."""
    o, d = pixel_ray(camera, width, height, x, y)              # refuses a pixel outside the viewport before anything is set
    ctx = _query_target(owner, scene_data, lds)
    hit = ctx.trace_rays(make_rays(o, d[None, :], 1000.0), lds=bool(lds))[0]
    if int(hit["sphere"]) == _abi.MIRT_RAY_MISS:
        return None
    return {"sphere": int(hit["sphere"]), "t": float(hit["t"]), "point": hit["point"].copy(), "normal": hit["normal"].copy()}


def _features(owner, spp: int, seed: int, width: int, height: int, camera: _abi.MirtGpuCamera, scene_data, lds: bool = False) -> dict:
    """Layer.features / Raytracer.features: Context.render_features of the whole viewport with `camera` -> the planes {"albedo"
    [h, w, 3], "normal" [h, w, 3], "t" [h, w], "sphere" [h, w]}.  Like _pick: a resident LDS scene -- or none yet -- is set again as a
    MIRT_SCENE_HBM scene first unless lds=True (_query_target), and on a node member 0's context renders the whole band."""
    if not isinstance(spp, (int, np.integer)) or isinstance(spp, bool) or int(spp) < 0:
        raise ValueError(f"spp must be a sample count >= 0, not {spp!r}")
    ctx = _query_target(owner, scene_data, lds)
    ctx.set_camera(camera)                                     # Layer.update_camera changes the camera without a device call
    rec = ctx.render_features(make_params(width, height, int(spp), mode=_abi.MIRT_MODE_PT, seed=seed), lds=bool(lds))
    return {k: rec[k].copy() for k in ("albedo", "normal", "t", "sphere")}


def _radiance(owner, rays, spp: int, seed: int, num_bounces: int, hosek: bool, scene_data, sort: bool = False, pool: bool = False, lds: bool = False) -> np.ndarray:
    """Layer.radiance / Raytracer.radiance: Context.trace_radiance of `rays` (RADIANCE_RAY_DTYPE: make_radiance_rays) -> float64 means
    [n, 3]; sort=True: in an order derived on the device (MIRT_RADIANCE_SORT), the same means.  Like _pick: a resident LDS scene -- or none yet -- is set again as a MIRT_SCENE_HBM scene first, and on a node the query
    runs on member 0's context.  lds=True: _query_target."""
    ctx = _query_target(owner, scene_data, lds)
    return radiance_mean(ctx.trace_radiance(rays, spp, num_bounces=num_bounces, seed=seed, hosek=hosek, sort=sort, pool=pool, lds=bool(lds)))


def _jpeg_check(rc: int) -> None:
    if rc != 0:
        raise MirtError(rc, (lib().mirt_jpeg_last_error() or b"").decode())


def jpeg_info(data: bytes) -> Tuple[int, int]:
    """(width, height) of a JPEG file's frame header."""
    w, h = C.c_uint32(), C.c_uint32()
    _jpeg_check(lib().mirt_jpeg_info(data, len(data), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def decode_jpeg(data: bytes) -> np.ndarray:
    """JPEG file bytes -> uint8 [h, w, 3] with the library's decoder (no device involved)."""
    w, h = jpeg_info(data)
    out = np.empty((h, w, 3), dtype=np.uint8)
    _jpeg_check(lib().mirt_jpeg_decode_rgb8(data, len(data), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def asset_path(name: str) -> str:
    """Resolve the reference's hard-coded asset paths (layer.rs:97,108) to the decoded texel tables that
    ship as package data (weekend-raytracer-wgpu_amd/assets/, written by tools/make_texture_fixtures.py),
    unless the file itself exists relative to the CWD."""
    if Path(name).exists():
        return name
    return str(Path(__file__).resolve().parent / "assets" / _ASSET_FIXTURES.get(name, name))


# ------------------------------------------------------------------------------------------------
# Layer — src/raytracer/layer.rs:37-282 (UI upload paths omitted: out of scope)
# ------------------------------------------------------------------------------------------------

class Layer:
    def __init__(self, size, render_params: RenderParams, *, device: int = 0, scene: Optional[Scene] = None,
                 devices: Optional[Sequence[int]] = None):
        # layer.rs:49-88.  `devices`: set_data renders through a Node on those devices (one frame cut across its members)
        # instead of one Context on `device`; the image is the same.
        self.vp_size = [float(f32(size[0])), float(f32(size[1]))]
        self.camera = GpuCamera.new(render_params.camera, (int(self.vp_size[0]), int(self.vp_size[1])))
        sc = scene if scene is not None else Layer.scene()
        self.world: List[Sphere] = list(sc.spheres)
        self.materials = list(sc.materials)
        self.global_texture_data = np.zeros((0, 3), dtype=np.float32)
        self.material_data: List[_abi.MirtMaterial] = []
        self.texture_id = 0
        self._device = device
        self._ctx: Optional[Context] = None
        self._devices = list(devices) if devices is not None else None
        self._node: Optional[Node] = None
        self._rgba: Optional[np.ndarray] = None
        self._hbm = False               # the context / node holds a MIRT_SCENE_HBM scene (move_spheres updates it in place)
        self.last_stats: Optional[dict] = None

    @staticmethod
    def new(size, render_params: RenderParams, **kw) -> "Layer":
        return Layer(size, render_params, **kw)

    @staticmethod
    def scene() -> Scene:                             # layer.rs:90-123
        materials = [
            Material.Checkerboard(even=Texture.new_from_color((0.5, 0.7, 0.8)),
                                  odd=Texture.new_from_color((0.9, 0.9, 0.9))),
            Material.Lambertian(albedo=Texture.new_from_image(asset_path("assets/moon.jpeg"))),
            Material.Metal(albedo=Texture.new_from_color((1.0, 0.85, 0.57)), fuzz=0.4),
            Material.Dielectric(refraction_index=1.5),
            Material.Lambertian(albedo=Texture.new_from_image(asset_path("assets/earthmap.jpeg"))),
        ]
        spheres = [
            Sphere.new((5.0, 1.2, -1.5), 1.2, 4),
            Sphere.new((0.0, -500.0, -1.0), 500.0, 0),
            Sphere.new((0.0, 1.0, 0.0), 1.0, 3),
            Sphere.new((-5.0, 1.0, 0.0), 1.0, 2),
            Sphere.new((2.0, -1.0, 0.0), 2.0, 3),
            Sphere.new((5.0, 0.8, 1.5), 0.8, 1),
        ]
        return Scene(spheres, materials)

    def set_global_data(self) -> bool:                # layer.rs:125-148
        self.material_data, self.global_texture_data = flatten_materials(self.materials)
        return True

    def scene_data(self) -> SceneData:
        """The bytes handed across the FFI: `world` (Vec<Box<Sphere>>) gathered contiguously."""
        return SceneData(self.camera.c, [s.to_c() for s in self.world], list(self.material_data),
                         self.global_texture_data)

    def set_data(self, render_params: RenderParams) -> None:   # layer.rs:264-282 -> ONE FFI call
        w, h = int(self.vp_size[0]), int(self.vp_size[1])
        params = make_params(w, h, render_params.sampling.num_samples_per_pixel, mode=_abi.MIRT_MODE_PARITY)
        if self._devices is not None:
            if self._node is None:
                self._node = Node(self._devices)
            self._hbm = set_scene_any_size(self._node, self.scene_data())
            self._rgba = self._node.render(params)
            self.last_stats = self._node.stats()
            return
        if self._ctx is None:
            self._ctx = Context(self._device)
        self._hbm = set_scene_any_size(self._ctx, self.scene_data())       # worlds beyond the LDS budget: MIRT_SCENE_HBM
        self._rgba = self._ctx.render(params)
        self.last_stats = self._ctx.stats()

    def move_spheres(self, first: int, spheres: Sequence[Sphere], render_params: Optional[RenderParams] = None) -> None:
        """Spheres first .. first + len(spheres) of `world` take the centre and the radius of `spheres` (they keep their material).
        After a set_data whose world went to device memory (MIRT_SCENE_HBM) the resident scene is updated in place and its BVH
        refitted (mirt_ctx_update_spheres / mirt_node_update_spheres); any other resident scene is set again; before the first
        set_data only `world` changes.  With `render_params` the image is rendered again, as set_data does.  `world` changes only
        when the device call succeeded."""
        first, moved = _moved(self.world, first, spheres)
        target = self._node if self._devices is not None else self._ctx
        if target is not None:
            _move_resident(self, target, first, moved,
                           lambda: SceneData(self.camera.c, [s.to_c() for s in _spliced(self.world, first, moved)], list(self.material_data),
                                             self.global_texture_data))
        self.world[first:first + len(moved)] = moved
        if target is not None and render_params is not None:
            w, h = int(self.vp_size[0]), int(self.vp_size[1])
            self._rgba = target.render(make_params(w, h, render_params.sampling.num_samples_per_pixel, mode=_abi.MIRT_MODE_PARITY))
            self.last_stats = target.stats()

    def set_world(self, spheres: Sequence[Sphere], render_params: Optional[RenderParams] = None) -> None:
        """`world` becomes `spheres` (any count; their material indices are taken).  After a set_data whose world went to device
        memory (MIRT_SCENE_HBM) the resident scene gets the new sphere table and a tree built on the device (mirt_ctx_set_spheres /
        mirt_node_set_spheres: materials and texels are not uploaded again); any other resident scene is set again; before the first
        set_data only `world` changes.  With `render_params` the image is rendered again, as set_data does.  `world` changes only
        when the device call succeeded."""
        new = _world(spheres)
        target = self._node if self._devices is not None else self._ctx
        if target is not None:
            _set_world_resident(self, target, new,
                                lambda: SceneData(self.camera.c, [s.to_c() for s in new], list(self.material_data), self.global_texture_data))
        self.world = new
        if target is not None and render_params is not None:
            w, h = int(self.vp_size[0]), int(self.vp_size[1])
            self._rgba = target.render(make_params(w, h, render_params.sampling.num_samples_per_pixel, mode=_abi.MIRT_MODE_PARITY))
            self.last_stats = target.stats()

    def _pick_target(self):
        if self._devices is not None:
            if self._node is None:
                self._node = Node(self._devices)
            return self._node
        if self._ctx is None:
            self._ctx = Context(self._device)
        return self._ctx

    def pick(self, x: int, y: int, *, lds: bool = False) -> Optional[dict]:
        """The sphere of `world` under pixel (x, y) of the viewport (row 0 on top): {"sphere": index into `world`, "t", "point",
        "normal"} -- exactly the record Context.trace_rays returns for the pinhole ray through the pixel's centre (pixel_ray) with
        t_max = 1000 -- or None where the ray leaves the scene.  Ray queries need the world in device memory: if the resident scene is
        not a MIRT_SCENE_HBM one (or nothing is resident yet, before the first set_data) the world is set as one first, and
        move_spheres / set_world then work on it in place; the next set_data sets the scene by its own rule again (a small world goes
        back to LDS), so a pick after it pays for one more set_scene.  lds=True (MIRT_QUERY_LDS): a world held in LDS stays there and
        answers from there, the same record; it needs a resident scene (after the first set_data)."""
        return _pick(self, x, y, int(self.vp_size[0]), int(self.vp_size[1]), self.camera.c, self.scene_data, lds)

    def features(self, spp: int = 0, *, seed: int = 0, lds: bool = False) -> dict:
        """What the camera sees first at every pixel of the viewport: {"albedo" [h, w, 3], "normal" [h, w, 3], "t" [h, w], "sphere"
        [h, w] (index into `world`, MIRT_RAY_MISS where the pixel's centre ray leaves the scene)} by Context.render_features with the
        layer's current camera.  spp = 0: the centre rays alone (an id and depth buffer for picking, exact guides); spp >= 1: albedo
        and normal are means over the path tracer's own primary rays of samples 0 .. spp - 1 (its pixel filter and depth of field).
        Like pick, it needs the world in device memory and sets it as a MIRT_SCENE_HBM scene first where it is not, unless lds=True
        (as in pick: the same planes from the scene in LDS)."""
        return _features(self, spp, seed, int(self.vp_size[0]), int(self.vp_size[1]), self.camera.c, self.scene_data, lds)

    def radiance(self, rays, spp: int = 16, *, seed: int = 0, num_bounces: int = 8, sort: bool = False, pool: bool = False, lds: bool = False) -> np.ndarray:
        """Path-traced radiance of `world` along rays the caller chooses (make_radiance_rays: panorama and fisheye cameras, probes)
        -> float64 means [n, 3] over samples 0 .. spp - 1 of every ray's stream, by Context.trace_radiance.  Like pick, it needs the
        world in device memory and sets it as a MIRT_SCENE_HBM scene first where it is not.  sort=True traces the batch in an order
        derived on the device: for rays that are not in a coherent order (probe grids, shuffled batches); the means are the same.
        pool=True asks for the pooled schedule (MIRT_RADIANCE_POOL, a hint): the means are the same.  lds=True: as in pick -- the same
        means from the scene in LDS, where `sort` and `pool` are ignored."""
        return _radiance(self, rays, spp, seed, num_bounces, False, self.scene_data, sort, pool, lds)

    def register_texture(self) -> np.ndarray:         # layer.rs:150-176: the RGBA8 bytes imgui would receive
        if self._rgba is None:
            raise RuntimeError("set_data has not been called")
        return self._rgba

    def imgbuf(self) -> Optional[np.ndarray]:         # layer.rs:182-186: ImageBuffer<Rgb<u8>>, [h][w][3]
        if self._rgba is None:
            return None
        h, w, _ = self._rgba.shape
        rgb = np.empty((h, w, 3), dtype=np.uint8)
        check(lib().mirt_rgba8_to_rgb8(self._rgba.ctypes.data_as(C.c_void_p), h * w, rgb.ctypes.data_as(C.c_void_p)))
        return rgb

    def update_camera(self, render_params: RenderParams) -> None:   # layer.rs:188-193 (does NOT re-render)
        self.camera = GpuCamera.new(render_params.camera, render_params.viewport_size)

    def resize(self, render_params: RenderParams) -> None:          # layer.rs:240-262
        width, height = render_params.viewport_size
        if self.vp_size[0] != float(width) or self.vp_size[1] != float(height):
            self.vp_size = [float(width), float(height)]
            self.camera = GpuCamera.new(render_params.camera, render_params.viewport_size)
            self.set_data(render_params)

    def close(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        if self._node is not None:
            self._node.close()
            self._node = None


# ------------------------------------------------------------------------------------------------
# Raytracer — the path-traced mode behind the names of src/raytracer/mod.rs:20-394
# (wgpu plumbing omitted; `render` = all frames of the progressive loop in one launch)
# ------------------------------------------------------------------------------------------------

class Raytracer:
    def __init__(self, scene: Scene, render_params: RenderParams, *, device: int = 0,
                 sky_state: Optional[_abi.MirtSkyState] = None, reference_stream: bool = False,
                 devices: Optional[Sequence[int]] = None):
        """`devices`: the render loop runs through a Node on those devices (every frame cut across its members, each member keeping
        the exact sums of its part) instead of one Context on `device`; the images are the same.

        `reference_stream=True` makes `render_frame` (and `render`) draw the samples of one frame from ONE RNG
        stream per pixel, seeded with the frame number -- the reference's initRng / samplePixel (wgsl:498-502,
        105-122) for `num_samples_per_pixel` samples per frame (MirtParams.frame_spp).  The default keeps one stream
        per sample (frame_number = sample + 1), which does not depend on how samples are grouped into frames.

        The reference's `frame_number` starts at 1 (mod.rs:284), advances with EVERY `render_frame` call -- frames that add nothing
        because the accumulation is complete included (mod.rs:350) -- and is not reset by `render_progress.reset()` (mod.rs:385).
        This class counts the same way (`frame_number`), and an accumulation that starts after k earlier frames seeds its j-th frame
        with frame k + j + 1 (MirtParams.frame_begin = k), so a camera move mid-session continues the reference's streams."""
        render_params.validate()                                   # mod.rs:44-47
        self.reference_stream = reference_stream
        self.render_params = render_params
        self.material_data, self.global_texture_data = flatten_materials(scene.materials)   # mod.rs:160-183
        self.spheres = list(scene.spheres)
        self.camera = GpuCamera.new(render_params.camera, render_params.viewport_size)
        self.sky_state = sky_state
        self._ctx = Node(list(devices)) if devices is not None else Context(device)    # the same calls on either
        self._on_node = devices is not None
        self._hbm = set_scene_any_size(self._ctx, self.scene_data())   # worlds beyond the LDS budget: MIRT_SCENE_HBM
        self._frames_queued = 0         # render_frame_device: frame k goes to frame stream k & 1
        self.last_stats: Optional[dict] = None
        self._accumulated = None        # RenderProgress (mod.rs:615-679): None = reset pending
        self.frame_number = 1           # mod.rs:284; advanced by every render_frame call (mod.rs:350), never reset
        self._frame_begin = 0           # frames rendered before the current accumulation started
        self._last_seed = 0             # of the last progressive frame or adaptive call: denoised() takes its guides with it
        self._temporal = None           # temporal_frame: the planes, the stream and the history it holds
        self._temporal_calls = 0        # temporal_frame: calls so far (frame k draws under seed + k)

    def scene_data(self) -> SceneData:
        return SceneData(self.camera.c, [s.to_c() for s in self.spheres], list(self.material_data),
                         self.global_texture_data, self.sky_state)

    def _params(self, spp: int, seed: int, flags: int, frame_begin: Optional[int] = None) -> _abi.MirtParams:
        rp = self.render_params
        if self.sky_state is not None:
            flags |= _abi.MIRT_FLAG_SKY_HOSEK
        if frame_begin is None:
            frame_begin = self._frame_begin
        return make_params(rp.viewport_size[0], rp.viewport_size[1], spp, mode=_abi.MIRT_MODE_PT,
                           num_bounces=rp.sampling.num_bounces, flags=flags, seed=seed,
                           frame_spp=rp.sampling.num_samples_per_pixel if self.reference_stream else 0,
                           frame_begin=frame_begin if self.reference_stream else 0)

    def _next_frame(self, seed: int, flags: int) -> _abi.MirtParams:
        """`RenderProgress::next_frame` (mod.rs:626-670): the params of the frame call to issue now -- `num_samples_per_pixel` samples
        until `max_samples_per_pixel` is reached, then spp = 0 (show the mean, add nothing: mod.rs:350).  Clears the sums first
        after a reset."""
        smp = self.render_params.sampling
        self._last_seed = seed
        if self._accumulated is None:                          # first frame after a reset: clear
            self._frame_begin = self.frame_number - 1          # this accumulation's frames are frame_number, frame_number + 1, ...
            self._ctx.accum_reset(self._params(smp.num_samples_per_pixel, seed, flags))
            self._accumulated = 0
        spp = smp.num_samples_per_pixel if self._accumulated + smp.num_samples_per_pixel <= smp.max_samples_per_pixel else 0
        return self._params(spp, seed, flags)

    def _frame_issued(self, params: _abi.MirtParams) -> None:
        self._accumulated += params.spp
        self.frame_number += 1                                 # mod.rs:350: also when the accumulation was complete already

    def render_frame(self, *, seed: int = 0, flags: int = 0) -> np.ndarray:
        """`Raytracer::render_frame` (mod.rs:303-351) without the wgpu draw: ONE frame call (one kernel launch) adds
        `num_samples_per_pixel` samples and returns the current estimate as RGBA8; once `max_samples_per_pixel` is reached the
        call adds nothing and returns the mean."""
        params = self._next_frame(seed, flags)
        img = self._ctx.accum_frame(params)
        self._frame_issued(params)
        return img

    def render_frame_device(self, d_out: int, stream: Optional[int] = None, *, seed: int = 0, flags: int = 0) -> int:
        """The same frame into device memory at address `d_out` (height x width x 4 bytes), asynchronously: for hosts that draw
        from device memory.  Returns the stream handle the frame is ordered on: wait on it before reading `d_out`.
        On a context `stream=None` alternates between its two frame streams (mirt_ctx_frame_stream), so that a host with two
        framebuffers keeps two frames in flight: pass framebuffer k & 1 for call k.  On a node the caller passes a stream of its
        own on member 0's device (the node's own stream has no handle to wait on): `stream=None` raises ValueError."""
        if self._on_node:
            if stream is None:
                raise ValueError("render_frame_device on a node needs a stream of the caller's (on member 0's device) to wait on")
        elif stream is None:
            stream = self._ctx.frame_stream(self._frames_queued & 1)
        params = self._next_frame(seed, flags)
        self._ctx.accum_frame_device(params, d_out, stream)
        if not self._on_node:
            self._frames_queued += 1
        self._frame_issued(params)
        return stream

    def progress(self) -> float:                               # mod.rs:390-393
        return (self._accumulated or 0) / float(self.render_params.sampling.max_samples_per_pixel)

    def set_render_params(self, render_params: RenderParams) -> None:   # mod.rs:353-388
        render_params.validate()
        self.render_params = render_params
        self.camera = GpuCamera.new(render_params.camera, render_params.viewport_size)
        self._ctx.set_camera(self.camera.c)
        self._accumulated = None                               # render_progress.reset() mod.rs:385

    def move_spheres(self, first: int, spheres: Sequence[Sphere]) -> None:
        """Spheres first .. first + len(spheres) of the scene take the centre and the radius of `spheres` (they keep their material).
        A scene in device memory (MIRT_SCENE_HBM) is updated in place and its BVH refitted on the device (mirt_ctx_update_spheres);
        any other scene is set again.  The progressive accumulation restarts, as the reference's does on any scene change
        (`render_progress.reset()`).  The held spheres change only when the device call succeeded."""
        first, moved = _moved(self.spheres, first, spheres)
        _move_resident(self, self._ctx, first, moved,
                       lambda: SceneData(self.camera.c, [s.to_c() for s in _spliced(self.spheres, first, moved)], list(self.material_data),
                                         self.global_texture_data, self.sky_state))
        self.spheres[first:first + len(moved)] = moved
        self._accumulated = None
        self._drop_history()

    def set_world(self, spheres: Sequence[Sphere]) -> None:
        """The scene's spheres become `spheres` (any count; their material indices are taken).  A scene in device memory
        (MIRT_SCENE_HBM) gets the new sphere table in place and a tree built on the device (mirt_ctx_set_spheres /
        mirt_node_set_spheres); any other scene is set again.  The progressive accumulation restarts.  The held spheres change only
        when the device call succeeded."""
        new = _world(spheres)
        _set_world_resident(self, self._ctx, new,
                            lambda: SceneData(self.camera.c, [s.to_c() for s in new], list(self.material_data), self.global_texture_data,
                                              self.sky_state))
        self.spheres = new
        self._accumulated = None
        self._drop_history()

    def _pick_target(self):
        return self._ctx

    def pick(self, x: int, y: int, *, lds: bool = False) -> Optional[dict]:
        """The sphere of the scene under pixel (x, y) of the viewport, as Layer.pick: {"sphere", "t", "point", "normal"} of the pinhole
        ray through the pixel's centre (the lens is ignored), or None.  A scene held in LDS is set again as a MIRT_SCENE_HBM scene
        first and stays one; the accumulation is not touched (the images are the same either way).  lds=True (MIRT_QUERY_LDS) leaves
        a scene held in LDS where it is and asks it there -- the same record, and later render() and progressive frames keep their
        LDS builds; on a scene that is already an HBM scene it changes nothing."""
        w, h = self.render_params.viewport_size
        return _pick(self, x, y, int(w), int(h), self.camera.c, self.scene_data, lds)

    def features(self, spp: Optional[int] = None, *, seed: int = 0, lds: bool = False) -> dict:
        """First-hit guides of the current viewport and camera, as Layer.features: {"albedo", "normal", "t", "sphere"} planes.
        spp = None takes `sampling.num_samples_per_pixel`, the samples of one displayed frame (samples 0 .. spp - 1 of `seed`, one RNG
        stream per sample whatever `reference_stream` says: a guide needs the frame's pixel filter, not its draws); spp = 0 the centre
        rays alone.  A scene held in LDS is set again as a MIRT_SCENE_HBM scene first and stays one; the accumulation is not touched.
        lds=True: as in pick -- the same planes from the scene in LDS, which stays there."""
        w, h = self.render_params.viewport_size
        if spp is None:
            spp = self.render_params.sampling.num_samples_per_pixel
        return _features(self, spp, seed, int(w), int(h), self.camera.c, self.scene_data, lds)

    def radiance(self, rays, spp: Optional[int] = None, *, seed: int = 0, sort: bool = False, pool: bool = False, lds: bool = False) -> np.ndarray:
        """Path-traced radiance of the scene along rays the caller chooses (make_radiance_rays) -> float64 means [n, 3], as
        Layer.radiance.  spp = None takes `sampling.num_samples_per_pixel`; the bounces are `sampling.num_bounces` and the sky is the
        scene's (the Hosek blob where there is one).  The accumulation is not touched.  sort, pool: as Layer.radiance.  lds=True: as in
        pick -- the same means from the scene in LDS, which stays there (`sort` and `pool` are ignored on it)."""
        if spp is None:
            spp = self.render_params.sampling.num_samples_per_pixel
        return _radiance(self, rays, spp, seed, self.render_params.sampling.num_bounces, self.sky_state is not None, self.scene_data, sort, pool, lds)

    def _default_adapt_run(self, ctx, step: int, max_spp: int, pool: bool, hosek: bool):
        """The MirtAdaptRun of render_adaptive(run=True): enough steps for a pixel that takes `step` samples at a time to reach `max_spp`
        and one more, steps that may grow to 8 x step, and min_items = the paths the device keeps in flight at once, times 2 --
        compute units x resident waves per unit x paths per wave (the pool's slots, or 64 lanes of 20 waves without a pool).  The
        factors 8 and 2 are guesses: nobody has tuned them."""
        import torch
        from .context import adapt_pool_plan, make_adapt_run
        cus = int(torch.cuda.get_device_properties(int(ctx.device)).multi_processor_count)
        plan = adapt_pool_plan(ctx.bvh_info()["plan"]["max_depth"], hosek) if pool else {"slots": 0}
        in_flight = cus * (plan["waves_per_cu"] * plan["slots"] if plan["slots"] else 20 * 64)
        max_steps = -(-int(max_spp) // int(step)) + 1
        if max_steps > _abi.MIRT_ADAPT_RUN_MAX_STEPS:
            raise ValueError(f"max_spp {max_spp} in steps of {step} needs {max_steps} steps: a run holds {_abi.MIRT_ADAPT_RUN_MAX_STEPS}; pass a MirtAdaptRun")
        cap = int(step)
        while cap < 8 * int(step) and 2 * cap <= _abi.MIRT_MAX_SPP_PER_CALL:
            cap *= 2
        return make_adapt_run(max_steps, min(2 * in_flight, 0xffffffff), cap)

    def render_adaptive(self, tolerance: int, max_spp: int, step: int = 4, min_spp: int = 4, *, seed: int = 0, flags: int = 0, pool: bool = False,
                        run=None, lds: bool = False) -> tuple:
        """Adaptive sampling of the current viewport (mirt_ctx_adapt_*): steps of `step` (even) samples for the pixels that have not
        converged -- fewer than `min_spp` samples, or even and odd halves further apart than tolerance x 2^-16 of the mean -- until no
        pixel below `max_spp` is left -> (RGBA8 [h][w][4], samples per pixel uint32 [h][w]).  One RNG stream per sample whatever
        `reference_stream` says (a pixel's samples must be independent).  A scene held in LDS is set again as a MIRT_SCENE_HBM scene
        first and stays one; on a node member 0's context renders the whole viewport.  The accumulation is not touched.  The mean of
        a pixel that a stopping rule has stopped is slightly biased.  pool=True asks for the pooled schedule
        (MIRT_ADAPT_POOL, a hint): the image and the counts are the same.  lds=True (MIRT_ADAPT_LDS) leaves a scene held in LDS where it
        is and runs the steps there -- the same image and counts, and later render() and progressive frames keep their LDS builds; on a
        scene that is already an HBM scene it changes nothing, and `pool` is ignored on a scene in LDS.

        run: None is the loop above, driven by the host: a step, a read of the count, the next step.  A MirtAdaptRun (make_adapt_run)
        replaces it by ONE call that queues run.max_steps steps (mirt_ctx_adapt_run_device) whose sample counts the device chooses --
        `step` << k, growing as the list shrinks, up to run.max_spp -- and the method waits once, in the resolve.  Steps behind the
        first empty one change nothing; a run that is too short leaves pixels unconverged (Context.adapt_run_log() tells).  A pixel may
        end above `max_spp` by less than run.max_spp.  run=True builds a default (_default_adapt_run): min_items from the device's
        compute units and the plan's resident waves and slots, times a small factor that nobody has tuned."""
        from .context import make_adapt_params
        adapt = make_adapt_params(min_spp, max_spp, tolerance, pool, lds)
        self._last_seed = seed
        if run is not None and run is not True and not isinstance(run, _abi.MirtAdaptRun):
            raise ValueError(f"run must be None, True or a MirtAdaptRun (make_adapt_run builds one), not {run!r}")
        if not isinstance(step, (int, np.integer)) or isinstance(step, bool) or int(step) < 2 or int(step) % 2:
            raise ValueError(f"step must be an even sample count >= 2, not {step!r}")
        target = self._pick_target()
        if not self._hbm and not lds:
            target.set_scene(self.scene_data(), hbm=True)
            self._hbm = True
        ctx = target.context(0) if hasattr(target, "context") else target
        ctx.set_camera(self.camera.c)
        rp = self.render_params
        if self.sky_state is not None:
            flags |= _abi.MIRT_FLAG_SKY_HOSEK
        w, h = int(rp.viewport_size[0]), int(rp.viewport_size[1])
        params = make_params(w, h, int(step), mode=_abi.MIRT_MODE_PT, num_bounces=rp.sampling.num_bounces, flags=flags, seed=seed)
        ctx.adapt_reset(params)
        if run is not None:
            if run is True:
                run = self._default_adapt_run(ctx, int(step), int(max_spp), bool(pool) and self._hbm, self.sky_state is not None)
            ctx.adapt_run(params, adapt, run)
            return ctx.adapt_resolve(params), ctx.adapt_read()["samples"].reshape(h, w).copy()
        while True:
            ctx.adapt_step(params, adapt)
            if ctx.adapt_stats()["active"] == 0:
                break
        return ctx.adapt_resolve(params), ctx.adapt_read()["samples"].reshape(h, w).copy()

    def denoised(self, source: str = "accum", *, levels: int = 3, sigma_colour: float = 1.0, normal_log2: int = 5, f32: bool = False,
                 seed: Optional[int] = None, flags: int = 0) -> np.ndarray:
        """The frame accumulated so far (source "accum": what render_frame* has added since the last reset) or the records of the last
        render_adaptive (source "adapt"), through the edge-avoiding a-trous filter of mirt_ctx_denoise -> RGBA8 [h][w][4], or with
        f32=True the linear mean as float32 [h][w][4].  The guides are features() with the frame's `num_samples_per_pixel` and seed
        (seed=None: that of the last frame or adaptive call), taken with lds=True when the scene lives in LDS, so it stays there.  The
        sums, the records and the sample counts are not touched.  `flags`: MIRT_FLAG_NO_TONEMAP / MIRT_FLAG_NO_SRGB for the RGBA8 form.
        A spatial filter, not a learned denoiser: it removes noise where neighbours of the same sphere, orientation and colour exist
        (DESIGN.md 10.17 has what was measured).  Not available on a node: a member's tiles are not neighbours."""
        from .context import make_denoise_params
        if self._on_node:
            raise ValueError("denoised needs a single context: a node member's tiles are not neighbours in the image")
        if not isinstance(flags, (int, np.integer)) or isinstance(flags, bool) or int(flags) & ~(_abi.MIRT_FLAG_NO_TONEMAP | _abi.MIRT_FLAG_NO_SRGB):
            raise ValueError(f"flags must be a combination of MIRT_FLAG_NO_TONEMAP and MIRT_FLAG_NO_SRGB, not {flags!r}")
        d = make_denoise_params(source, levels=levels, sigma_colour=sigma_colour, normal_log2=normal_log2, f32=f32)
        if seed is None:
            seed = self._last_seed
        w, h = (int(v) for v in self.render_params.viewport_size)
        g = self.features(seed=seed, lds=not self._hbm)
        guides = np.zeros((h, w), FEATURE_DTYPE)
        for k in ("albedo", "normal", "t", "sphere"):
            guides[k] = g[k]
        return self._ctx.denoise(make_params(w, h, 0, mode=_abi.MIRT_MODE_PT, flags=int(flags)), d, guides)

    def _drop_history(self) -> None:
        """temporal_frame starts over: sphere ids may name other spheres now, or the planes have another size."""
        held = getattr(self, "_temporal", None)
        if held is not None:
            held["have"] = False

    def temporal_frame(self, *, seed: int = 0, levels: int = 3, sigma_colour: float = 1.0, normal_log2: int = 5, max_history: float = 4.0,
                       depth_tolerance: float = 0.05, clamp: bool = True, flags: int = 0) -> np.ndarray:
        """The frame of a MOVING camera -> RGBA8 [h][w][4]: `num_samples_per_pixel` fresh samples (every call resets the accumulation
        and draws under seed + the number of calls so far, so frames are independent), the guides of those samples, the a-trous filter
        of mirt_ctx_denoise to float32, and mirt_ctx_reproject against the history this object holds: the previous call's result,
        guides and camera.  The whole frame is queued on one stream through the _device forms into planes this object owns (two
        history planes and two guide planes, used alternately); the host waits once, for the RGBA8 copy.  The first call, and the
        first after set_world, move_spheres or a changed viewport size, has no history and returns the denoised frame;
        set_render_params with a new camera KEEPS the history.  Afterwards the accumulation is marked reset, so a progressive loop
        starts over.  A scene held in LDS stays there.  `flags`: MIRT_FLAG_NO_TONEMAP / MIRT_FLAG_NO_SRGB.  The gain over
        denoised() alone is modest (DESIGN.md 10.18 has what was measured); not available on a node."""
        import torch
        from .context import make_denoise_params, make_reproject_params
        if self._on_node:
            raise ValueError("temporal_frame needs a single context: a node member's tiles are not neighbours in the image")
        if not isinstance(flags, (int, np.integer)) or isinstance(flags, bool) or int(flags) & ~(_abi.MIRT_FLAG_NO_TONEMAP | _abi.MIRT_FLAG_NO_SRGB):
            raise ValueError(f"flags must be a combination of MIRT_FLAG_NO_TONEMAP and MIRT_FLAG_NO_SRGB, not {flags!r}")
        if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or int(seed) < 0:
            raise ValueError(f"seed must be an unsigned integer, not {seed!r}")
        w, h = (int(v) for v in self.render_params.viewport_size)
        cur_cam = _abi.MirtGpuCamera.from_buffer_copy(self.camera.c)
        to_f32 = make_denoise_params("accum", levels=levels, sigma_colour=sigma_colour, normal_log2=normal_log2, f32=True)
        to_rgba8 = make_denoise_params("accum", levels=levels, sigma_colour=sigma_colour, normal_log2=normal_log2)
        lds = not self._hbm
        ctx = _query_target(self, self.scene_data, lds)
        n = w * h
        T = self._temporal
        if T is None or T["size"] != (w, h):
            dev = f"cuda:{int(ctx.device)}"
            plane = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev)
            T = self._temporal = {"size": (w, h), "have": False, "cur": 0, "camera": None, "stream": torch.cuda.Stream(device=dev),
                                  "colour": plane(n * 16), "history": [plane(n * 16), plane(n * 16)], "guides": [plane(n * 32), plane(n * 32)],
                                  "rgba8": plane(n * 4)}
        repro = make_reproject_params(T["camera"] if T["have"] else cur_cam, cur_cam, max_history=max_history, depth_tolerance=depth_tolerance,
                                      clamp=clamp)                # (checks its arguments before anything is queued)
        st = int(T["stream"].cuda_stream)
        frame_seed = int(seed) + self._temporal_calls
        self._temporal_calls += 1
        cur = T["cur"] ^ 1
        guides, history, rgba8 = T["guides"][cur], T["history"][cur], T["rgba8"]

        self._accumulated = None                                  # every call starts a fresh accumulation
        params = self._next_frame(frame_seed, int(flags))
        ctx.set_camera(cur_cam)
        ctx.accum_frame_device(params, rgba8.data_ptr(), st)      # (its image is overwritten below)
        self._frame_issued(params)
        ctx.render_features_device(make_params(w, h, int(params.spp), mode=_abi.MIRT_MODE_PT, seed=frame_seed), guides.data_ptr(), n * 32, stream=st, lds=lds)
        tone = make_params(w, h, 0, mode=_abi.MIRT_MODE_PT, flags=int(flags))
        if T["have"]:
            ctx.denoise_device(tone, to_f32, guides.data_ptr(), n * 32, T["colour"].data_ptr(), n * 16, st)
            ctx.reproject_device(tone, repro, T["colour"].data_ptr(), guides.data_ptr(), T["history"][cur ^ 1].data_ptr(), T["guides"][cur ^ 1].data_ptr(),
                                 history.data_ptr(), n, d_out_rgba8=rgba8.data_ptr(), stream=st)
        else:                                                     # no history: the denoised frame is the history (its fourth channel is a length of 1)
            ctx.denoise_device(tone, to_f32, guides.data_ptr(), n * 32, history.data_ptr(), n * 16, st)
            ctx.denoise_device(tone, to_rgba8, guides.data_ptr(), n * 32, rgba8.data_ptr(), n * 4, st)
        T["cur"], T["camera"], T["have"] = cur, cur_cam, True
        self._accumulated = None                                  # a progressive loop restarts
        with torch.cuda.stream(T["stream"]):
            img = rgba8.cpu()                                     # ordered behind the frame on its stream; the one host wait
        return img.numpy().reshape(h, w, 4).copy()

    def temporal_history(self) -> Optional[np.ndarray]:
        """The history temporal_frame holds -> float32 [h][w][4] = {r, g, b, history length} (linear, before the tone curves), or None
        before the first frame and after the history was dropped."""
        T = self._temporal
        if T is None or not T["have"]:
            return None
        import torch
        w, h = T["size"]
        with torch.cuda.stream(T["stream"]):
            a = T["history"][T["cur"]].cpu()
        return a.numpy().view(np.float32).reshape(h, w, 4).copy()

    def render(self, *, seed: int = 0, flags: int = 0, frame_begin: int = 0) -> np.ndarray:
        """All `max_samples_per_pixel` samples in one launch -> RGBA8 [h][w][4].

        With `reference_stream=True` the launch is the accumulation a FRESH reference `Raytracer` would converge to: its frames are
        numbered frame_begin + 1, frame_begin + 2, ... with `frame_begin = 0` by default -- not the frame count of this object's
        progressive loop, so the image does not depend on earlier `render_frame` / `set_render_params` calls.  Pass
        `frame_begin=rt.frame_number - 1` for the accumulation the progressive loop would start NOW.  Ignored without
        `reference_stream` (one stream per sample)."""
        params = self._params(self.render_params.sampling.max_samples_per_pixel, seed, flags, frame_begin=frame_begin)
        img = self._ctx.render(params)
        self.last_stats = self._ctx.stats()                        # (a node: its MirtNodeStats)
        return img

    def close(self) -> None:
        self._ctx.close()                                          # (mirt_ctx_destroy waits for what temporal_frame queued)
        self._temporal = None


__all__ = ["Angle", "Camera", "GpuCamera", "SamplingParams", "SkyParams", "RenderParams",
           "RenderParamsValidationError", "FlyCameraController", "Sphere", "Texture", "Material",
           "TextureDescriptor", "GpuMaterial", "Scene", "Layer", "Raytracer", "flatten_materials",
           "asset_path", "MirtError", "decode_jpeg", "jpeg_info", "pixel_ray", "pixel_project"]
