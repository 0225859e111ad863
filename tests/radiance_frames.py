"""Whole frames as the judge of mirt_ctx_trace_radiance* (host-side data only; a helper like radiance_ref.py, not a conftest; nothing
here runs a kernel of the library except through the context a test hands to query_frame).

The header's contract: a ray equal to a renderer's primary ray, with `stream` equal to that pixel's index, continues that sample's
path bit for bit.  feature_ref.sample_rays restates the renderer's primary rays of ONE sample index in float32 (tests/test_gpu_features.py
holds it to the device bit for bit), so the oracle's render_pt_sums of a whole w x h frame at spp = 1, sample_begin = s is what a query
of frame_rays(cam, w, h, s) must return: w * h records for one oracle render, where the probe camera of radiance_ref.py costs one
render per ray.  The oracle's sums are additive over sample_begin (tests/test_radiance_frames_cpu.py), a jittered pixel's ray differs
from sample to sample, so several samples are several queries accumulated into the same records (query_frame).

High streams: a pixel of an 8 x 2^29 image's last row has index 0xFFFFFFF8 + x, and the oracle renders that row alone."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE
import feature_ref as fr
import hbm_worlds
import oracle_binding as ob
import radiance_ref as rr

HIGH_STREAM = 0xFFFFFFF8                    # the first pixel index of the last row of an 8 x 2^29 image
TALL = 1 << 29

_rays = {}


def frame_rays(cam, w, h, sample, seed=0) -> np.ndarray:
    """RADIANCE_RAY_DTYPE [w * h]: the renderer's primary rays of sample index `sample` of every pixel, row-major, stream = y * w + x.
    Computed once per argument set; the returned array is read-only."""
    key = (bytes(cam), int(w), int(h), int(sample), int(seed))
    if key not in _rays:
        ys, xs = np.divmod(np.arange(w * h), w)
        o, d = fr.sample_rays(cam, w, h, xs, ys, sample, seed)
        rays = m.make_radiance_rays(o, d, ys * w + xs)
        rays.flags.writeable = False
        _rays[key] = rays
    return _rays[key]


def _records(sums, samples) -> np.ndarray:
    out = np.zeros(len(sums), RADIANCE_DTYPE)
    out["sum"] = sums
    out["samples"] = samples
    return out


def frame_sums(scene_data, w, h, sample, num_bounces, seed=0, hosek=False, spp=1) -> np.ndarray:
    """uint64 [h, w, 3]: the oracle's sums of the frame at `spp` samples from sample index `sample`."""
    p = m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, num_bounces=num_bounces, sample_begin=sample, seed=seed,
                      flags=_abi.MIRT_FLAG_SKY_HOSEK if hosek else 0)
    return ob.render_pt_sums(scene_data, p)


def frame_records(scene_data, w, h, samples, num_bounces, seed=0, hosek=False) -> np.ndarray:
    """RADIANCE_DTYPE [w * h]: what query_frame must return -- the uint64 sum over s in `samples` of the oracle's 1-spp frame at
    sample_begin = s, and samples = len(samples)."""
    total = np.zeros((h, w, 3), np.uint64)
    for s in samples:
        total += frame_sums(scene_data, w, h, s, num_bounces, seed, hosek)
    return _records(total.reshape(-1, 3), len(samples))


def query_frame(ctx, cam, w, h, samples, **kw) -> np.ndarray:
    """One ctx.trace_radiance(frame_rays(.., s), 1, sample_begin=s, ..) per sample: the first overwrites, the later ones accumulate
    into its records -- with another ray array per call, the only way a query can follow a jittered pixel."""
    seed = kw.get("seed", 0)
    out = None
    for s in samples:
        got = ctx.trace_radiance(frame_rays(cam, w, h, s, seed), 1, sample_begin=s, into=out, **kw)
        assert out is None or got is out
        out = got
    return out


@functools.lru_cache(maxsize=None)
def high_stream_sums(i, spp=4, num_bounces=8, sample_begin=0, seed=0, hosek=False) -> np.ndarray:
    """uint64 [1, 8, 3]: the oracle's sums of ray i of radiance_ref.ray_set() for streams 0xFFFFFFF8 .. 0xFFFFFFFF -- the last row,
    and that row alone, of an 8 x 2^29 image seen through the ray's probe camera.  Computed once per argument set; read-only."""
    p = m.make_params(rr.N_STREAMS, TALL, spp, mode=m.MIRT_MODE_PT, num_bounces=num_bounces, sample_begin=sample_begin, seed=seed,
                      row_begin=TALL - 1, row_end=TALL, flags=_abi.MIRT_FLAG_SKY_HOSEK if hosek else 0)
    assert ob.out_rows(p) == 1 and ob.out_row_index(p, 0) == TALL - 1
    s = ob.render_pt_sums(rr.scene(i, rr.sky_blob() if hosek else None), p, n_threads=1)
    s.flags.writeable = False
    return s


def high_stream_records(i, **kw) -> np.ndarray:
    """RADIANCE_DTYPE [8]: what a query of high_stream_rays((i,)) must return."""
    return _records(high_stream_sums(int(i), **kw)[0], kw.get("spp", 4))


def high_stream_rays(rays_idx) -> np.ndarray:
    """radiance_ref.rays_and_streams(rays_idx) with streams 0xFFFFFFF8 + k in place of k."""
    rays = rr.rays_and_streams(rays_idx).copy()
    rays["stream"] += np.uint32(HIGH_STREAM)
    return rays


# ------------------------------------------------------------------------------------------ the worlds the frames are taken of

SUBSET = (0, 1, 5, 6, rr.INSIDE_HERO, rr.MISSES_ALL, 30, 31)      # tests/test_gpu_trace_radiance.py's: ground, small spheres, glass, inside the hero, sky, ...
DEEP_W, DEEP_H = 48, 32                                            # tests/test_gpu_deep_trees.py's viewport
DEEP_FRAMES = (("stair32", "far"), ("line32", "near"), ("line32", "long"))      # the frames the CPU audit looks at
SMALL_W, SMALL_H = 16, 8


def fixture_scene_of(arr, aperture=0.0, sky=None):
    """The feature fixture's camera, materials and texels over another sphere table."""
    mats, tex = fr.fixture().mats, fr.fixture().tex
    return hbm_worlds.scene_from_arrays(fr.fixture_camera(aperture), arr, mats, tex, sky)


def fixture_scene_with_sky():
    return fixture_scene_of(fr.fixture().arr, sky=rr.sky_blob())


def moved_fixture_world(seed=11) -> np.ndarray:
    """The fixture world with every small sphere moved and resized by tests/test_gpu_update_spheres.py's jitter; the ground and the
    heroes stay."""
    from test_gpu_update_spheres import _jitter
    arr = fr.fixture().arr
    out = _jitter(arr, seed)
    out[:5] = arr[:5]
    return out


def deep_cameras(name) -> dict:
    """view -> camera: every view tests/test_gpu_deep_trees.py renders a world of tests/deep_worlds.py from."""
    import deep_worlds as dw
    if name in dw.STAIRS:
        return {"far": dw.staircase_camera(DEEP_W, DEEP_H)}
    return {"near": dw.line_camera(DEEP_W, DEEP_H), "long": dw.line_camera_long(dw.ray_set(name)[0], DEEP_W, DEEP_H)}


def deep_scene(name, cam, sky=None):
    import deep_worlds as dw
    mats, tex = hbm_worlds.field_materials()
    return hbm_worlds.scene_from_arrays(cam, dw.ray_set(name)[0], mats, tex, sky)


def degenerate_camera():
    return hbm_worlds.look(SMALL_W, SMALL_H, (0, 1.5, 5), (0, 1, 0), vfov=40)


def degenerate_worlds() -> dict:
    """The empty table, one sphere (a leaf root) and 1000 copies of that sphere."""
    one = hbm_worlds.sphere_array([[0.0, 1.0, 0.0]], [1.0], [0])
    return {"empty": one[:0], "one sphere": one, "1000 copies": np.tile(one, 1000)}


def degenerate_scene(arr):
    mats, tex = hbm_worlds.field_materials()
    return hbm_worlds.scene_from_arrays(degenerate_camera(), arr, mats, tex)
