"""The CPU reference of mirt_ctx_render_features* and the fixture its tests share (host-side data only; a helper like
ray_query_ref.py, not a conftest).  Nothing here runs a kernel of the library.

Rays: the RNG floats of a sample are oracle_binding.rng_stream(x + y * width, sample, seed, 4) = {jitter u, jitter v, lens radius,
lens angle}; the centre ray takes 0.5 for both jitter values and no lens.  Arithmetic is float32 throughout, fused only where the
kernels write fma (grid_rounding.fma32); the lens uses IEEE sqrt and the oracle's sincos of f32(2 pi) * r3, and is skipped by the
pinhole shortcut's rule (lens_radius == 0, a finite lens basis and a finite eye without a -0 component: the origin is the eye).
Hits: ray_query_ref.trace_ref with t_max = 1000 -- the flat scan restated.  Albedo: (u, v) from the oracle's acos and atan2 as
albedo_at writes them, texture_lookup restated (clamp, saturating conversion, offset + i * w + j, the index clamped to the table),
the checkerboard's side from the oracle's sin_sign.  Accumulation: float32 sums from +0 in sample order, then one division.
Comparison: by bit pattern with NaN equal to NaN (same_bits)."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd.context import FEATURE_DTYPE
import hbm_worlds
import oracle_binding as ob
import ray_query_ref as rq
from grid_rounding import fma32

f32 = np.float32
MISS = 0xFFFFFFFF
PI, FRAC_1_PI, TWO_PI = f32(3.1415927), f32(0.31830987), f32(6.2831855)
MISSING_ALBEDO = np.array([0.9921, 0.24705, 0.57254], f32)


# ------------------------------------------------------------------------------------------ rays

def _cam(cam):
    g = lambda a: np.asarray(a[:3], f32)
    return dict(eye=g(cam.eye), hor=g(cam.horizontal), ver=g(cam.vertical), llc=g(cam.lower_left_corner), u=g(cam.u), v=g(cam.v),
                lens_radius=f32(cam.lens_radius))


def is_pinhole(cam) -> bool:
    c = _cam(cam)
    if c["lens_radius"] != 0:
        return False
    fin = np.isfinite(c["u"]).all() and np.isfinite(c["v"]).all() and np.isfinite(c["eye"]).all()
    return bool(fin and not ((c["eye"] == 0) & np.signbit(c["eye"])).any())


def _through(c, u, v, origin):
    """direction = fma(v, ver, fma(u, hor, llc)) - origin per component, float32."""
    return np.stack([(fma32(v, np.full_like(v, c["ver"][k]), fma32(u, np.full_like(u, c["hor"][k]), np.full_like(u, c["llc"][k])))
                      - origin[:, k]).astype(f32) for k in range(3)], 1)


def _uv(w, h, xs, ys, ju, jv):
    inv_w, inv_h = f32(1.0) / f32(w), f32(1.0) / f32(h)
    u = ((xs.astype(f32) + ju).astype(f32) * inv_w).astype(f32)
    v = (f32(1.0) - ((ys.astype(f32) + jv).astype(f32) * inv_h).astype(f32)).astype(f32)
    return u, v


def centre_rays(cam, w, h, xs, ys):
    """(origins, directions) [n, 3] float32 of the centre rays of pixels (xs, ys)."""
    c = _cam(cam)
    half = np.full(len(xs), 0.5, f32)
    u, v = _uv(w, h, np.asarray(xs), np.asarray(ys), half, half)
    o = np.broadcast_to(c["eye"], (len(u), 3)).astype(f32)
    return o, _through(c, u, v, o)


def sample_rays(cam, w, h, xs, ys, sample, seed):
    """(origins, directions) of the renderer's primary rays of sample index `sample` of pixels (xs, ys)."""
    c = _cam(cam)
    xs, ys = np.asarray(xs), np.asarray(ys)
    r = np.stack([ob.rng_stream(int(x) + int(y) * w, int(sample), int(seed), 4) for x, y in zip(xs, ys)]).astype(f32)
    u, v = _uv(w, h, xs, ys, r[:, 0], r[:, 1])
    o = np.broadcast_to(c["eye"], (len(u), 3)).astype(f32)
    if not is_pinhole(cam):
        with np.errstate(all="ignore"):
            lr = np.sqrt(r[:, 2]).astype(f32)
            s, co = ob.sincos((TWO_PI * r[:, 3]).astype(f32))
            lpx = (c["lens_radius"] * (lr * co).astype(f32)).astype(f32)
            lpy = (c["lens_radius"] * (lr * s).astype(f32)).astype(f32)
            off = np.stack([fma32(lpy, np.full_like(lpy, c["v"][k]), (lpx * c["u"][k]).astype(f32)) for k in range(3)], 1)
            o = (o + off).astype(f32)
    return o, _through(c, u, v, o)


# ------------------------------------------------------------------------------------------ albedo

def _clamp01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, f32(0), np.where(x > 1, f32(1), x)).astype(f32)           # a NaN stays


def _sat_u32(x):
    """Rust `as u32`: truncate, saturate, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, x, f32(0)).astype(np.float64)
    return np.where(c >= 4294967296.0, 0xFFFFFFFF, np.minimum(c, 4294967295.0).astype(np.uint64)).astype(np.uint64)


def texture_lookup(tex, desc, u, v):
    """texels [n, 3] of descriptor (width, height, offset) at (u, v)."""
    w, h, off = (int(x) for x in desc)
    with np.errstate(invalid="ignore"):
        j = _sat_u32((_clamp01(u) * f32(w)).astype(f32))
        i = _sat_u32(((f32(1.0) - _clamp01(v)).astype(f32) * f32(h)).astype(f32))
    idx = (i * np.uint64(w) + j) & np.uint64(0xFFFFFFFF)              # the kernels index in 32 bits
    g = np.minimum(idx + np.uint64(off), np.uint64(len(tex) - 1))
    return np.asarray(tex, f32).reshape(-1, 3)[g.astype(np.int64)]


def albedo_ref(mats, tex, midx, hp, hn):
    """The attenuation of the scatter routine of materials mats[midx] at hit points hp with normals hn, [n, 3] float32."""
    out = np.zeros((len(midx), 3), f32)
    with np.errstate(all="ignore"):
        theta = ob.acos((-hn[:, 1]).astype(f32))
        phi = (ob.atan2((-hn[:, 2]).astype(f32), hn[:, 0].astype(f32)) + PI).astype(f32)
        u = ((f32(0.5) * FRAC_1_PI) * phi).astype(f32)
        v = (FRAC_1_PI * theta).astype(f32)
        sgn = [ob.sin_sign((f32(5.0) * hp[:, k]).astype(f32)) for k in range(3)]
    negative = (sgn[0] * sgn[1] * sgn[2]) < 0
    for k in np.unique(midx):
        sel = np.nonzero(midx == k)[0]
        mat = mats[int(k)]
        d1 = (mat.desc1.width, mat.desc1.height, mat.desc1.offset)
        d2 = (mat.desc2.width, mat.desc2.height, mat.desc2.offset)
        if mat.id in (0, 1):
            out[sel] = texture_lookup(tex, d1, u[sel], v[sel])
        elif mat.id == 2:
            out[sel] = f32(1.0)
        elif mat.id == 3:
            out[sel] = np.where(negative[sel, None], texture_lookup(tex, d1, u[sel], v[sel]), texture_lookup(tex, d2, u[sel], v[sel]))
        else:
            out[sel] = MISSING_ALBEDO
    return out


# ------------------------------------------------------------------------------------------ frames

class FeatureRef:
    """The reference frames of one world, camera and viewport.  A layer -- the hits, normals and albedos of one ray per pixel of the
    whole viewport: the centre rays (sample None) or those of one sample index and seed -- is computed once and shared by every frame
    that needs it; frames are assembled from layers in sample order."""

    def __init__(self, arr, mats, tex, cam, w, h):
        self.arr, self.mats, self.tex, self.cam, self.w, self.h = arr, list(mats), np.asarray(tex, f32).reshape(-1, 3), cam, int(w), int(h)
        self.cen, self.rad = rq.world_arrays(arr)
        ys, xs = np.divmod(np.arange(self.w * self.h), self.w)
        self.xs, self.ys = xs, ys
        self._layers = {}

    def rays(self, sample=None, seed=0):
        """(origins, directions) of the whole viewport: the centre rays (sample None) or those of one sample index and seed."""
        if sample is None:
            return centre_rays(self.cam, self.w, self.h, self.xs, self.ys)
        return sample_rays(self.cam, self.w, self.h, self.xs, self.ys, sample, seed)

    def layer(self, sample=None, seed=0):
        key = (sample, seed if sample is not None else 0)
        if key not in self._layers:
            o, d = self.rays(sample, seed)
            hits = rq.trace_ref(o, d, 1000.0, self.cen, self.rad)
            hit = hits["sphere"] != MISS
            alb = np.zeros((len(o), 3), f32)
            h = np.nonzero(hit)[0]
            if len(h):
                alb[h] = albedo_ref(self.mats, self.tex, self.arr["material_idx"][hits["sphere"][h]], hits["point"][h], hits["normal"][h])
            lay = dict(rays=(o, d), hits=hits, hit=hit, albedo=alb)
            for a in (o, d, hits, hit, alb):
                a.setflags(write=False)
            self._layers[key] = lay
        return self._layers[key]

    def frame(self, spp=0, sample_begin=0, seed=0) -> np.ndarray:
        """FEATURE_DTYPE [h, w]: the whole viewport."""
        centre = self.layer()
        out = np.zeros(self.w * self.h, FEATURE_DTYPE)
        out["sphere"] = centre["hits"]["sphere"]
        out["t"] = centre["hits"]["t"]                              # 0 for a miss, as trace_ref leaves it
        sum_n, sum_a = np.zeros((len(out), 3), f32), np.zeros((len(out), 3), f32)
        layers = [centre] if spp == 0 else [self.layer(sample_begin + s, seed) for s in range(spp)]
        with np.errstate(all="ignore"):
            for lay in layers:
                h = lay["hit"]
                sum_n[h] = (sum_n[h] + lay["hits"]["normal"][h]).astype(f32)
                sum_a[h] = (sum_a[h] + lay["albedo"][h]).astype(f32)
            n = f32(max(spp, 1))
            out["normal"] = (sum_n / n).astype(f32)
            out["albedo"] = (sum_a / n).astype(f32)
        return out.reshape(self.h, self.w)

    def of(self, params) -> np.ndarray:
        """FEATURE_DTYPE [rows, w]: the rows `params` selects, compact."""
        assert (params.width, params.height) == (self.w, self.h)
        full = self.frame(int(params.spp), int(params.sample_begin), int(params.seed))
        rows = [m.params_out_row_index(params, i) for i in range(m.params_out_rows(params))]
        return full[rows]


def same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Per record (any shape): every 32-bit word equal, a NaN counting as equal to any NaN; `sphere` (word 7) is an integer."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    nan = np.isnan(g.view(f32)) & np.isnan(w.view(f32))
    nan[:, 7] = False
    return ((g == w) | nan).all(1).reshape(np.shape(got))


# ------------------------------------------------------------------------------------------ the fixture

W, H = 67, 45
IMAGE_MATERIAL = 1          # hbm_worlds.field_materials(): the lambertian with the earth map


def fixture_camera(aperture=0.0):
    return hbm_worlds.look(W, H, (13, 2, 3), (0, 0.5, 0), vfov=25, aperture=aperture)


@functools.lru_cache(maxsize=None)
def fixture(aperture=0.0) -> FeatureRef:
    """rtiow_field(3000) seen through a 67 x 45 viewport: the width is no multiple of 64, so every wave boundary falls inside a row
    and the last wave has dead lanes."""
    arr, mats, tex = rq.field_world()
    return FeatureRef(arr, mats, tex, fixture_camera(aperture), W, H)


def fixture_scene(aperture=0.0):
    arr, mats, tex = rq.field_world()
    return hbm_worlds.scene_from_arrays(fixture_camera(aperture), arr, mats, tex)
