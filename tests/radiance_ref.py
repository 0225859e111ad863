"""The independent judge of mirt_ctx_trace_radiance* and the seeded ray set its tests use (host-side data only; a helper like
ray_query_ref.py, not a conftest).

The judge is the CPU oracle's path tracer, reached through its camera.  A MirtGpuCamera with horizontal = vertical = u = v = 0,
lens_radius = 0, eye = o and lower_left_corner = fl32(o + d) makes every primary ray of every pixel and sample the ONE ray
(o, fl32(llc - o)), whatever the jitter and the lens draws are, while every pixel keeps its own RNG stream (seeded by its index) and
still consumes the four draws of a primary ray.  So `oracle_binding.render_pt_sums` of an n x 1 image with that camera gives, for
pixel p, exactly the sums a radiance query must return for that ray with stream = p."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE
import hbm_worlds
import oracle_binding as ob
import ray_query_ref as rq

f32 = np.float32
N_RAYS, N_STREAMS = 32, 8
SEED = 0x1234_5678_9ABC_DEF0                # both 32-bit halves of the 64-bit seed are mixed in
INSIDE_HERO, MISSES_ALL = 26, 27            # rays of ray_set() placed by hand: see there
BOUNCE_RAYS = (8, 21, MISSES_ALL, 30)       # the four rays of the bounce-limit test: two whose paths outlast 8 segments, the sky, the missing material


@functools.lru_cache(maxsize=None)
def world():
    """hbm_worlds.rtiow_field(300): (spheres, materials, texels) -- all five routines, a missing-material id, a hollow glass hero."""
    return hbm_worlds.rtiow_field(300)


def probe_camera(o, llc) -> _abi.MirtGpuCamera:
    """The camera whose every primary ray is (o, fl32(llc - o)): everything else zero."""
    c = _abi.MirtGpuCamera()
    for k in range(3):
        c.eye[k] = float(o[k])
        c.lower_left_corner[k] = float(llc[k])
    return c


@functools.lru_cache(maxsize=None)
def ray_set():
    """(origins [32, 3], directions [32, 3], lower-left corners [32, 3]) float32.  26 seeded rays (np.random.default_rng(3): origins
    uniform in [-6, 6] x [0.3, 3] x [-6, 6], directions normal with y replaced by -0.3 |y|: they look across the field and slightly
    down), then six placed by hand: one that starts inside the hollow glass hero (inside its inner sphere of radius -0.9), one that
    points at the sky and misses everything, one each aimed at the two other heroes (image-textured lambertian, metal), and one each
    that comes down on the first small sphere with the missing-material id and on the first with a plain lambertian.
    Every direction is fl32(fl32(o + d0) - o), the ray the probe camera makes, so that oracle and query trace the same bits."""
    arr, _, _ = world()
    rng = np.random.default_rng(3)
    n = N_RAYS - 6
    o = np.stack([rng.uniform(-6, 6, n), rng.uniform(0.3, 3, n), rng.uniform(-6, 6, n)], 1)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -0.3 * np.abs(d[:, 1])
    above = np.array([0.25, 3.0, 0.125])
    small = [arr["center"][5 + int(np.nonzero(arr["material_idx"][5:] == k)[0][0]), :3].astype(np.float64) for k in (6, 0)]
    o = np.concatenate([o, [[0.25, 1.125, 0.0], [2.0, 2.5, 7.0], [-4.0, 1.5, 6.0], [7.0, 2.0, 5.0], small[0] + above, small[1] + above]]).astype(f32)
    d = np.concatenate([d, [[1.0, 0.25, 0.5], [0.125, 1.0, 0.25], [0.0, -0.5, -6.0], [-3.0, -1.0, -5.0], -above, -above]]).astype(f32)
    llc = (o + d).astype(f32)
    return o, (llc - o).astype(f32), llc


def scene(i: int, sky=None):
    """The world with ray i's probe camera (what the ORACLE renders; a query's scene may carry any camera)."""
    arr, mats, tex = world()
    o, _, llc = ray_set()
    return hbm_worlds.scene_from_arrays(probe_camera(o[i], llc[i]), arr, mats, tex, sky)


@functools.lru_cache(maxsize=None)
def oracle_sums(i: int, spp: int = 4, num_bounces: int = 8, sample_begin: int = 0, seed: int = 0, hosek: bool = False) -> np.ndarray:
    """uint64 [N_STREAMS, 3]: the oracle's exact sums of ray i for streams 0 .. N_STREAMS - 1.  Computed once per argument set; the
    returned array is read-only."""
    p = m.make_params(N_STREAMS, 1, spp, mode=m.MIRT_MODE_PT, num_bounces=num_bounces, sample_begin=sample_begin, seed=seed,
                      flags=_abi.MIRT_FLAG_SKY_HOSEK if hosek else 0)
    s = ob.render_pt_sums(scene(i, sky_blob() if hosek else None), p, n_threads=1)[0]
    s.flags.writeable = False
    return s


def oracle_records(rays_idx, **kw) -> np.ndarray:
    """RADIANCE_DTYPE [len(rays_idx) * N_STREAMS]: what a query of rays_and_streams(rays_idx) must return."""
    spp = kw.get("spp", 4)
    out = np.zeros(len(rays_idx) * N_STREAMS, RADIANCE_DTYPE)
    out["sum"] = np.concatenate([oracle_sums(int(i), **kw) for i in rays_idx])
    out["samples"] = spp
    return out


def rays_and_streams(rays_idx) -> np.ndarray:
    """RADIANCE_RAY_DTYPE [len(rays_idx) * N_STREAMS]: every ray of rays_idx with streams 0 .. N_STREAMS - 1, ray-major."""
    o, d, _ = ray_set()
    idx = np.repeat(np.asarray(rays_idx, np.int64), N_STREAMS)
    return m.make_radiance_rays(o[idx], d[idx], np.tile(np.arange(N_STREAMS), len(rays_idx)))


@functools.lru_cache(maxsize=None)
def first_hits() -> np.ndarray:
    """RAY_HIT_DTYPE [32]: what every ray of the set hits first, by the CPU restatement of the flat scan (ray_query_ref.trace_ref)."""
    arr, _, _ = world()
    o, d, _ = ray_set()
    return rq.trace_ref(o, d, 1000.0, *rq.world_arrays(arr))


@functools.lru_cache(maxsize=None)
def sky_blob() -> _abi.MirtSkyState:
    """A MirtSkyState for the Hosek cases.  Any blob serves: oracle and kernel evaluate the same 36 words."""
    sky = _abi.MirtSkyState()
    for c in range(3):
        for i, v in enumerate([-1.1, -0.3, 0.5, 1.2, -2.5, 0.4, 0.2, 1.5, 0.6]):
            sky.params[9 * c + i] = v * (1.0 + 0.1 * c)
        sky.radiances[c] = 1.0 + c
    sky.sun_direction[:] = [0.0, 0.6, 0.8, 0.0]
    return sky
