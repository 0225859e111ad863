"""The sort code of MIRT_RAYS_SORT / MIRT_RADIANCE_SORT restated in numpy from the text of include/mirt.h, and the ray sets the two
test files of the feature share (host-side data only; a helper like ray_query_ref.py, not a conftest).

Every line of `codes` is one float32 operation on float32 operands, which numpy rounds once, as IEEE 754 asks: the restatement is
bit-exact by construction and has nothing in common with the library's C++ but the header's text.

D: the rays of a 67 x 45 fisheye camera with a 180 degree field of view over the fixture world -- one origin, 3 015 pairwise distinct
codes (asserted in tests/test_ray_sort_abi.py), so the sorted order of D does not depend on the order D is handed over in.
T: 3 015 copies of one ray -- all ties, so the order is the identity."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
import feature_ref as fr
import hbm_worlds
import ray_query_ref as rq

f32 = np.float32
ORIGIN_BITS, DIRECTION_BITS = 5, 8
N = fr.W * fr.H                       # 3 015: 47 full waves and one of 7 live lanes (11 full blocks of 256 and one of 199 threads)
D_FOV = 180.0                         # degrees across the width of D's fisheye: 120 to 270 give 3 015 distinct codes, 90 and 300 do not
D_EYE, D_AT = (13, 2, 3), (0, 0.5, 0)  # the fixture camera's
SIZES = (1, 63, 64, 65, 257, N)


def _q(f, n):
    """0 for anything that is not above 0 (NaN included), n - 1 from n on, truncation between."""
    f = np.asarray(f, f32)
    with np.errstate(invalid="ignore"):
        pos, top = f > f32(0.0), f >= f32(n)
    mid = np.where(pos & ~top, f, f32(0.0)).astype(f32)
    return np.where(top, np.uint32(n - 1), np.where(pos, mid.astype(np.uint32), np.uint32(0))).astype(np.uint32)


def codes(centre, radius, o, d) -> np.ndarray:
    """uint32 [n]: the 31-bit codes of rays (o, d) [n, 3] under the bounds (centre [3], radius)."""
    o, d = np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3)
    centre, radius = np.asarray(centre, f32), f32(radius)
    with np.errstate(all="ignore"):
        inv = f32(16.0) / radius
        c = []
        for k in range(3):
            lo = centre[k] - radius
            c.append(_q(((o[:, k] - lo).astype(f32) * inv).astype(f32), 1 << ORIGIN_BITS))
        ax, ay, az = (np.abs(d[:, k]) for k in range(3))
        s = ((ax + ay).astype(f32) + az).astype(f32)
        r = (f32(1.0) / s).astype(f32)
        u, v = (d[:, 0] * r).astype(f32), (d[:, 1] * r).astype(f32)
        one, neg = f32(1.0), f32(-1.0)
        fu = ((one - np.abs(v)).astype(f32) * np.where(u >= 0, one, neg)).astype(f32)
        fv = ((one - np.abs(u)).astype(f32) * np.where(v >= 0, one, neg)).astype(f32)
        fold = d[:, 2] < 0
        u, v = np.where(fold, fu, u).astype(f32), np.where(fold, fv, v).astype(f32)
        half = f32(1 << (DIRECTION_BITS - 1))
        a = _q(((u * half).astype(f32) + half).astype(f32), 1 << DIRECTION_BITS)
        b = _q(((v * half).astype(f32) + half).astype(f32), 1 << DIRECTION_BITS)
    m3 = np.zeros(len(o), np.uint32)
    m2 = np.zeros(len(o), np.uint32)
    for j in range(ORIGIN_BITS):
        m3 |= (((c[0] >> j) & 1) << (3 * j + 2)) | (((c[1] >> j) & 1) << (3 * j + 1)) | (((c[2] >> j) & 1) << (3 * j))
    for j in range(DIRECTION_BITS):
        m2 |= (((a >> j) & 1) << (2 * j + 1)) | (((b >> j) & 1) << (2 * j))
    return ((m3 << np.uint32(2 * DIRECTION_BITS)) | m2).astype(np.uint32)


def order_of(code) -> np.ndarray:
    """Ascending (code, index): the stable argsort."""
    return np.argsort(np.asarray(code), kind="stable").astype(np.uint32)


def world_bounds(arr):
    """(centre float32 [3], radius float32): a sphere around the world's finite spheres, for the tests that have no resident tree to
    ask (any bounds define a code; a context's own are those of bvh_info)."""
    cen, rad = rq.world_arrays(arr)
    ok = np.isfinite(cen).all(1) & np.isfinite(rad)
    lo, hi = (cen[ok] - np.abs(rad[ok])[:, None]).min(0), (cen[ok] + np.abs(rad[ok])[:, None]).max(0)
    return ((lo + hi) * f32(0.5)).astype(f32), f32(np.linalg.norm((hi - lo).astype(np.float64)) * 0.5)


def d_directions(fov_degrees=D_FOV):
    """float32 [N, 3]: an equidistant fisheye of 67 x 45 pixels at the fixture camera's eye, looking where it looks; `fov_degrees`
    across the width, the same angle per pixel down the height.  (No pinhole camera does for D: from this eye a 67 x 45 pinhole frame
    has at most 2 918 distinct codes, at 70 degrees -- narrower and the pixels are closer than the octahedral cells, wider and the
    corners crowd.)"""
    eye, at = np.array(D_EYE, np.float64), np.array(D_AT, np.float64)
    fwd = (at - eye) / np.linalg.norm(at - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    ys, xs = np.divmod(np.arange(N), fr.W)
    per = np.radians(fov_degrees) / fr.W
    px, py = (xs + 0.5 - fr.W / 2) * per, (fr.H / 2 - ys - 0.5) * per
    th, ph = np.hypot(px, py), np.arctan2(py, px)
    d = (np.sin(th) * np.cos(ph))[:, None] * right + (np.sin(th) * np.sin(ph))[:, None] * up + np.cos(th)[:, None] * fwd
    return d.astype(f32)


@functools.lru_cache(maxsize=None)
def set_d():
    """(origins, directions) of D, row-major; read-only."""
    d = d_directions()
    o = np.tile(np.array(D_EYE, f32), (N, 1))
    o.flags.writeable = d.flags.writeable = False
    return o, d


@functools.lru_cache(maxsize=None)
def set_t():
    """(origins, directions) of T: ray 1 507 of D, 3 015 times."""
    o, d = set_d()
    return np.tile(o[N // 2], (N, 1)), np.tile(d[N // 2], (N, 1))


def permutation(n, seed=2024) -> np.ndarray:
    return np.random.default_rng(seed).permutation(n)
