"""Worlds beyond the LDS budget for the MIRT_SCENE_HBM tests (host-side data only): seeded fields and soups built with numpy and
handed to SceneData as one ctypes array (a million Python MirtSphere objects would take longer to build than to render)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi

SPHERE_DTYPE = np.dtype([("center", "<f4", (4,)), ("radius", "<f4"), ("material_idx", "<u4"), ("_pad", "<u4", (2,))])
assert SPHERE_DTYPE.itemsize == C.sizeof(_abi.MirtSphere)


def sphere_array(centres, radii, mats) -> np.ndarray:
    a = np.zeros(len(radii), SPHERE_DTYPE)
    a["center"][:, :3] = np.asarray(centres, np.float32)
    a["radius"] = np.asarray(radii, np.float32)
    a["material_idx"] = np.asarray(mats, np.uint32)
    return a


def c_spheres(arr: np.ndarray):
    """ctypes view (no copy) of a SPHERE_DTYPE array; keep `arr` alive with it."""
    arr = np.ascontiguousarray(arr)
    return (_abi.MirtSphere * max(1, len(arr))).from_buffer(arr if len(arr) else np.zeros(1, SPHERE_DTYPE)), arr


def scene_from_arrays(camera, arr: np.ndarray, mats, tex, sky=None) -> "m.SceneData":
    sd = m.SceneData(camera, [], list(mats), tex, sky)
    carr, keep = c_spheres(arr)
    sd.spheres = carr if len(arr) else []
    sd._c_spheres = carr
    sd._keep = keep
    return sd


def field_materials():
    """All five routines: lambertian (colour and image texture), metal, dielectric, checkerboard, and a missing-material id (4)."""
    mats = [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))),
            m.Material.Lambertian(albedo=m.Texture.new_from_image(m.asset_path("assets/earthmap.jpeg"))),
            m.Material.Metal(albedo=m.Texture.new_from_color((0.7, 0.6, 0.5)), fuzz=0.2),
            m.Material.Dielectric(refraction_index=1.5),
            m.Material.Checkerboard(even=m.Texture.new_from_color((0.2, 0.3, 0.1)), odd=m.Texture.new_from_color((0.9, 0.9, 0.9))),
            m.Material.Lambertian(albedo=m.Texture.new_from_color((0.8, 0.3, 0.2)))]
    gm, tex = m.flatten_materials(mats)
    bad = _abi.MirtMaterial()           # GpuMaterial id 7: scatterRay's default branch (shade_missing)
    bad.id = 7
    bad.desc1.width, bad.desc1.height, bad.desc1.offset = 0, 0, 0xffffffff
    bad.desc2.width, bad.desc2.height, bad.desc2.offset = 0, 0, 0xffffffff
    return list(gm) + [bad], tex


def rtiow_field(n: int, seed: int = 1):
    """An RTIOW-style field of n spheres: a ground sphere, three heroes (one a hollow glass: an inner sphere of negative radius), and
    small spheres of every material scattered over a square whose side grows with sqrt(n)."""
    rng = np.random.default_rng(seed)
    k = n - 5
    side = 0.9 * np.sqrt(k)
    xz = rng.uniform(-side, side, (k, 2))
    r = rng.uniform(0.15, 0.25, k)
    cen = np.stack([xz[:, 0], r, xz[:, 1]], 1)
    mat = rng.integers(0, 7, k)
    cen = np.concatenate([[[0, -1000, 0], [0, 1, 0], [0, 1, 0], [-4, 1, 0], [4, 1, 0]], cen])
    rad = np.concatenate([[1000.0, 1.0, -0.9, 1.0, 1.0], r])
    mats = np.concatenate([[4, 3, 3, 1, 2], mat])
    mats_c, tex = field_materials()
    return sphere_array(cen, rad, mats), mats_c, tex


def clustered_soup(n: int, seed: int = 2, clusters: int = 24):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-30, 30, (clusters, 3))
    which = rng.integers(0, clusters, n)
    cen = centres[which] + rng.normal(0, 2.0, (n, 3))
    rad = rng.uniform(0.05, 0.3, n)
    mats_c, tex = field_materials()
    return sphere_array(cen, rad, rng.integers(0, 7, n)), mats_c, tex


def look(w: int, h: int, eye, at, vfov=30.0, aperture=0.0, focus=10.0):
    eye = np.asarray(eye, np.float32)
    d = (np.asarray(at, np.float32) - eye).astype(np.float32)
    cam = m.Camera(eye, d / np.float32(np.linalg.norm(d)), np.asarray((0, 1, 0), np.float32), m.Angle.degrees(vfov), aperture, focus)
    return m.GpuCamera.new(cam, (w, h)).c
