"""mirt_ctx_trace_radiance* on the device: radiance_rays_kernel<HOSEK, BVH> against the CPU oracle's path tracer, reached through a
camera that makes every primary ray the one ray under test (tests/radiance_ref.py), record by record and bit by bit, for the tree
(host-built and device-built) and the flat scan.  One context for the module; the oracle computes a ray's sums once per argument set
and shares them (radiance_ref.oracle_sums is cached and read-only).  That the ray set exercises what it is meant to is asserted on
the oracle alone in tests/test_trace_radiance_abi.py."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE, RADIANCE_RAY_DTYPE
import hbm_worlds
import radiance_ref as rr
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

f32 = np.float32
BVH = pytest.mark.parametrize("bvh", ["host", "device"])
ALL = tuple(range(rr.N_RAYS))
SUBSET = (0, 1, 5, 6, rr.INSIDE_HERO, rr.MISSES_ALL, 30, 31)      # ground, small spheres, glass, inside the hero, sky, missing material, lambertian
FOUR = rr.BOUNCE_RAYS


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _set(ctx, bvh="host", sky=None, arr=None):
    world, mats, tex = rr.world()
    ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), world if arr is None else arr, mats, tex, sky),
                  hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _tree_and_flat(ctx, rays, spp, what, hosek=False, **kw):
    """The tree's records, after checking that the flat scan on the device returns the same bytes."""
    tf = ("false", "true")
    tree = ctx.trace_radiance(rays, spp, hosek=hosek, **kw)
    assert ctx.last_kernel() == f"radiance_rays_kernel<{tf[hosek]},true>"
    flat = ctx.trace_radiance(rays, spp, hosek=hosek, flat=True, **kw)
    assert ctx.last_kernel() == f"radiance_rays_kernel<{tf[hosek]},false>"
    assert tree.dtype == RADIANCE_DTYPE and tree.shape == flat.shape == (len(rays),)
    differ = np.nonzero((_bytes(tree).reshape(-1, 32) != _bytes(flat).reshape(-1, 32)).any(1))[0]
    print(f"{what}: tree and flat differ in {len(differ)} of {len(rays)} records")
    assert len(differ) == 0, f"{what}: tree != flat at ray {differ[0]}: tree {tree[differ[0]]}, flat {flat[differ[0]]}"
    return tree


def _agree(got, want, what):
    bad = np.nonzero((_bytes(got).reshape(-1, 32) != _bytes(want).reshape(-1, 32)).any(1))[0]
    print(f"{what}: {len(got)} records, {len(bad)} differ from the oracle")
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(got)} records differ, first: ray {bad[0] // rr.N_STREAMS} of the query, stream "
                           f"{bad[0] % rr.N_STREAMS}: got {got[bad[0]]}, want {want[bad[0]]}")


# ---- 1. the oracle's sums ----

@BVH
def test_records_equal_the_oracles_sums(ctx, bvh):
    _set(ctx, bvh)
    got = _tree_and_flat(ctx, rr.rays_and_streams(ALL), 4, f"32 rays x 8 streams, {bvh} tree")
    _agree(got, rr.oracle_records(ALL), f"32 rays x 8 streams, {bvh} tree")
    # another first sample and a seed with both halves set
    got = _tree_and_flat(ctx, rr.rays_and_streams(SUBSET), 4, f"sample_begin 5 and a seed, {bvh} tree", sample_begin=5, seed=rr.SEED)
    _agree(got, rr.oracle_records(SUBSET, sample_begin=5, seed=rr.SEED), f"sample_begin 5 and a seed, {bvh} tree")
    for only in (dict(sample_begin=5), dict(seed=rr.SEED), dict(seed=rr.SEED & 0xFFFFFFFF), dict(seed=rr.SEED >> 32 << 32)):
        other = rr.oracle_records(SUBSET, sample_begin=5, seed=rr.SEED)
        assert not np.array_equal(_bytes(rr.oracle_records(SUBSET, **only)), _bytes(other)), only   # each of them reaches the sums


@BVH
def test_hosek_sky_records_equal_the_oracles(ctx, bvh):
    _set(ctx, bvh, sky=rr.sky_blob())
    got = _tree_and_flat(ctx, rr.rays_and_streams(SUBSET), 4, f"Hosek sky, {bvh} tree", hosek=True)
    _agree(got, rr.oracle_records(SUBSET, hosek=True), f"Hosek sky, {bvh} tree")
    plain = ctx.trace_radiance(rr.rays_and_streams(SUBSET), 4)     # the same scene without the flag: the gradient sky
    _agree(plain, rr.oracle_records(SUBSET), "a scene with a blob, queried without the flag")
    assert not np.array_equal(_bytes(plain), _bytes(got))


# ---- 2. additivity ----

def test_accumulating_calls_add_up_to_one_call(ctx):
    _set(ctx)
    rays = rr.rays_and_streams(SUBSET)
    for flat in (False, True):
        whole = ctx.trace_radiance(rays, 5, flat=flat)
        _agree(whole, rr.oracle_records(SUBSET, spp=5), f"spp 5, flat {flat}")
        part = ctx.trace_radiance(rays, 2, flat=flat)
        assert (part["samples"] == 2).all()
        back = ctx.trace_radiance(rays, 3, sample_begin=2, flat=flat, into=part)
        assert back is part and np.array_equal(_bytes(part), _bytes(whole)) and (part["samples"] == 5).all()
    dirty = np.zeros(len(rays), RADIANCE_DTYPE)
    _bytes(dirty)[:] = 0xA5
    lib = m.lib()
    p = _abi.MirtRadianceParams(5, 0, 8, 0, 0)
    assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), len(rays), C.byref(p), C.c_void_p(dirty.ctypes.data)) == 0
    assert np.array_equal(_bytes(dirty), _bytes(whole)), "without MIRT_RADIANCE_ACCUMULATE the record is overwritten, _pad included"
    # ACCUMULATE reads what is there: 0xA5 patterns plus the sums, mod 2^64 and 2^32
    _bytes(dirty)[:] = 0xA5
    p.flags = _abi.MIRT_RADIANCE_ACCUMULATE
    assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), len(rays), C.byref(p), C.c_void_p(dirty.ctypes.data)) == 0
    assert np.array_equal(dirty["sum"], whole["sum"] + np.uint64(0xA5A5A5A5A5A5A5A5)) and (dirty["samples"] == (0xA5A5A5A5 + 5) % 2 ** 32).all()
    assert not dirty["_pad"].any()


# ---- 3. placement: sizes, order, the record behind the last ----

@pytest.mark.parametrize("flat", [False, True], ids=["tree", "flat"])
def test_a_record_depends_on_its_ray_alone(ctx, flat):
    _set(ctx)
    rays = np.concatenate([rr.rays_and_streams(ALL), rr.rays_and_streams(ALL[:1])[:1]])          # 257 rays
    want = np.concatenate([rr.oracle_records(ALL), rr.oracle_records(ALL[:1])[:1]])
    lib = m.lib()
    p = _abi.MirtRadianceParams(4, 0, 8, _abi.MIRT_RADIANCE_FLAT if flat else 0, 0)
    for n in (1, 63, 64, 65, 257):
        out = np.zeros(n + 1, RADIANCE_DTYPE)
        _bytes(out)[:] = 0xA5                                       # the canary: record n must stay as it is
        assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), n, C.byref(p), C.c_void_p(out.ctypes.data)) == 0, lib.mirt_last_error()
        _agree(out[:n], want[:n], f"n_rays {n}")
        assert (_bytes(out[n:]) == 0xA5).all(), f"n_rays {n}: the record behind the last was written"
    perm = np.random.default_rng(5).permutation(len(rays))
    _agree(ctx.trace_radiance(rays[perm], 4, flat=flat), want[perm], "a permutation of the batch")


# ---- 4. bounces ----

def test_bounce_limits(ctx):
    _set(ctx)
    rays = rr.rays_and_streams(ALL)
    for flat in (False, True):
        none = ctx.trace_radiance(rays, 4, num_bounces=0, flat=flat)
        assert not none["sum"].any() and (none["samples"] == 4).all() and not none["_pad"].any()
    four = rr.rays_and_streams(FOUR)
    for nb in (1, 300):
        got = _tree_and_flat(ctx, rays, 4, f"{nb} bounces", num_bounces=nb)
        of_four = got.reshape(rr.N_RAYS, rr.N_STREAMS)[list(FOUR)].reshape(-1)
        assert np.array_equal(_bytes(ctx.trace_radiance(four, 4, num_bounces=nb)), _bytes(of_four))      # alone or in the batch: the same records
        _agree(of_four, rr.oracle_records(FOUR, num_bounces=nb), f"{nb} bounces, four rays")
    one = ctx.trace_radiance(rays, 4, num_bounces=1).reshape(rr.N_RAYS, rr.N_STREAMS)
    hit = rr.first_hits()["sphere"] != rq.MISS
    assert not one["sum"][hit].any() and one["sum"][~hit].all()     # one segment: the sky where the ray leaves, nothing where it hits


# ---- 5. rays the renderer never makes ----

def test_rays_no_camera_makes_return_and_agree_between_tree_and_flat(ctx):
    _set(ctx)
    arr, _, _ = rr.world()
    o, d, defined = rq.degenerate_rays()                            # zero directions, zero components, NaN and infinite origins, 1e-20, 1e20
    nan_d = np.array([[np.nan, -1, 0], [1, np.inf, 0], [0, -np.inf, np.nan], [np.inf, np.inf, np.inf]], f32)
    o = np.concatenate([o, np.tile(o[:16], (4, 1))])
    d = np.concatenate([d, np.repeat(nan_d, 16, 0)])
    # origins on a sphere's surface, in float32: the metal hero (4, 1, 0) r = 1 and the ground sphere's top, leaving, grazing and entering
    on = np.array([[5, 1, 0], [4, 2, 0], [4, 1, -1], [3, 1, 0], [0.5, 0, 0.5]], f32)
    dirs = np.array([[1, 0.25, 0], [0, 1, 0], [0, 0, 1], [-1, -0.25, 0.5], [0, -1, 0], [0.5, 0, -1]], f32)
    o = np.concatenate([o, np.repeat(on, len(dirs), 0)]).astype(f32)
    d = np.concatenate([d, np.tile(dirs, (len(on), 1))]).astype(f32)
    rays = m.make_radiance_rays(o, d, np.arange(len(o)) % 7)
    for nb in (1, 8):
        got = _tree_and_flat(ctx, rays, 2, f"{len(rays)} degenerate rays, {nb} bounces", num_bounces=nb)
        assert (got["samples"] == 2).all()
    zero = ~(d != 0).any(1)
    assert zero.sum() >= 128 and np.isnan(d).any() and np.isinf(d).any() and np.isnan(o).any() and np.isinf(o).any()


# ---- 6. the device form, the state a query leaves alone, errors ----

def _device_query(ctx, torch, rays, stream, offset=0, preset=0x5A, **kw):
    """trace_radiance_device between torch buffers (4-byte aligned at `offset`) on a caller stream -> the records."""
    n = len(rays)
    buf = np.zeros(32 * n + 16, np.uint8)
    buf[offset:offset + 32 * n] = _bytes(rays)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(buf).to("cuda:0", non_blocking=False)
        d_out = torch.full((32 * n + 32 + 16,), preset, dtype=torch.uint8, device="cuda:0")
        ctx.trace_radiance_device(d_rays.data_ptr() + offset, n, d_out.data_ptr() + offset, stream=stream.cuda_stream, **kw)
        out = d_out.cpu().numpy()                                   # ordered after the query on the same stream
    assert (out[:offset] == preset).all() and (out[offset + 32 * n:] == preset).all(), "bytes around the records were written"
    return out[offset:offset + 32 * n].copy().view(RADIANCE_DTYPE)


def test_device_form_on_a_caller_stream(ctx):
    import torch
    _set(ctx, "device")
    rays = np.concatenate([rr.rays_and_streams(ALL), rr.rays_and_streams(SUBSET)[:37]])          # 293 rays: two blocks, a ragged tail
    stream = torch.cuda.Stream(device="cuda:0")
    for flat in (False, True):
        host = ctx.trace_radiance(rays, 4, flat=flat)
        for offset in (0, 4):
            got = _device_query(ctx, torch, rays, stream, offset, spp=4, flat=flat)
            assert ctx.last_kernel() == f"radiance_rays_kernel<false,{'false' if flat else 'true'}>"
            assert np.array_equal(_bytes(got), _bytes(host)), (flat, offset)
    _agree(host[:256], rr.oracle_records(ALL), "the device form's batch")
    acc = _device_query(ctx, torch, rays, stream, 4, preset=0, spp=3, sample_begin=1, accumulate=True)    # zero records + samples 1 .. 3
    first = ctx.trace_radiance(rays, 1)
    assert np.array_equal(acc["sum"] + first["sum"], host["sum"]) and (acc["samples"] == 3).all()
    assert ctx.trace_stats()["kernel_ms"] > 0.0 and not any(v for k, v in ctx.trace_stats().items() if k != "kernel_ms")
    # the world replaced from device memory: the next query answers for the new world
    arr, _, _ = rr.world()
    fewer = np.concatenate([arr[:5], arr[40:200]])
    d_fewer = torch.from_numpy(_bytes(fewer).copy()).to("cuda:0")
    ctx.set_spheres_device(len(fewer), d_fewer.data_ptr())
    after = _tree_and_flat(ctx, rays, 4, "after set_spheres_device")
    assert not np.array_equal(_bytes(after), _bytes(host))
    assert np.array_equal(_bytes(_device_query(ctx, torch, rays, stream, spp=4)), _bytes(after))
    _set(ctx, "host", arr=fewer)
    assert np.array_equal(_bytes(ctx.trace_radiance(rays, 4)), _bytes(after))                   # a fresh scene of that world answers the same


def test_errors_and_untouched_state(ctx):
    lib = m.lib()
    rays = rr.rays_and_streams(SUBSET)
    out = np.zeros(len(rays), RADIANCE_DTYPE)
    _bytes(out)[:] = 0xA5
    pr, po, n = C.c_void_p(rays.ctypes.data), C.c_void_p(out.ctypes.data), len(rays)
    P = _abi.MirtRadianceParams
    both = lambda p, a=pr, b=po, k=n: (lib.mirt_ctx_trace_radiance(ctx._h, a, k, C.byref(p) if p is not None else None, b),
                                       lib.mirt_ctx_trace_radiance_device(ctx._h, a, k, C.byref(p) if p is not None else None, b, None))
    scene, cam = m.scenes.three_spheres()
    lds = m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))
    ctx.set_scene(lds)                                              # an LDS scene: nothing to query
    assert both(P(4, 0, 8, 0, 0)) == (_abi.MIRT_ERR_NO_SCENE,) * 2 and b"MIRT_SCENE_HBM" in lib.mirt_last_error()
    with pytest.raises(m.MirtError) as e:
        ctx.trace_radiance(rays, 4)
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    # a sphere whose material does not exist: the status a path-traced render gives
    arr, _, _ = rr.world()
    broken = arr.copy()
    broken["material_idx"][7] = 99
    _set(ctx, arr=broken)
    with pytest.raises(m.MirtError) as e:
        ctx.render(m.make_params(16, 8, 1, mode=m.MIRT_MODE_PT))
    assert e.value.status == _abi.MIRT_ERR_MATERIAL_INDEX
    assert both(P(4, 0, 8, 0, 0)) == (_abi.MIRT_ERR_MATERIAL_INDEX,) * 2
    assert len(ctx.trace_rays(rq.rays_of(rays["origin"], rays["direction"]))) == n               # ray queries read no material
    _set(ctx)
    assert both(P(4, 0, 8, _abi.MIRT_RADIANCE_SKY_HOSEK, 0)) == (_abi.MIRT_ERR_SKY,) * 2          # no blob in this scene
    for bad in (8, 1 << 31, 0xFFFFFFF8):
        assert both(P(4, 0, 8, bad, 0)) == (_abi.MIRT_ERR_BAD_MODE,) * 2
    assert both(P(0, 0, 8, 0, 0)) == (_abi.MIRT_ERR_SPP_ZERO,) * 2
    assert both(P((1 << 24) + 1, 0, 8, 0, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    assert both(P(4, 0xFFFFFFFD, 8, 0, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    for a, b in ((None, po), (pr, None), (None, None)):
        assert both(P(4, 0, 8, 0, 0), a, b) == (_abi.MIRT_ERR_NULL_POINTER,) * 2
    assert both(None) == (_abi.MIRT_ERR_NULL_POINTER,) * 2
    assert (_bytes(out) == 0xA5).all(), "a refused call writes nothing"
    assert both(P(4, 0, 8, 0, 0), None, None, 0) == (0, 0) and len(ctx.trace_radiance(rays[:0], 4)) == 0
    assert both(P(0, 0, 8, 0, 0), None, None, 0) == (_abi.MIRT_ERR_SPP_ZERO,) * 2                 # the checks come before "nothing to do"
    # a render, an accumulation -- and a query in between changes neither the statistics nor the sums nor the next render
    p = m.make_params(64, 48, 4, mode=m.MIRT_MODE_PT, num_bounces=4)
    img = ctx.render(p)
    kernel = ctx.last_kernel()
    ctx.accum_reset(p)
    ctx.accum_add(p)
    sums = ctx.accum_read(p)
    before = ctx.stats()
    assert before["samples"] == 64 * 48 * 4 and before["launches"] >= 2 and before["kernel_ms"] > 0
    got = ctx.trace_radiance(rays, 4)
    assert ctx.last_kernel() == "radiance_rays_kernel<false,true>" != kernel
    assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p), sums)
    after = ctx.stats()
    assert after["launches"] == 0 and after["kernel_ms_total"] == 0                                       # a query is no render launch
    assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
    assert np.array_equal(ctx.render(p), img)
    _agree(got, rr.oracle_records(SUBSET), "a query between renders")
    ctx.set_timing(False)
    ctx.trace_radiance(rays, 4)
    assert ctx.trace_stats()["kernel_ms"] == 0.0                    # kernel_ms follows mirt_ctx_set_timing
    ctx.set_timing(True)
    ctx.trace_radiance(rays, 4)
    st = ctx.trace_stats()
    assert st["kernel_ms"] > 0.0 and not any(v for k, v in st.items() if k != "kernel_ms")


# ---- 7. a renderer's primary ray continues that sample's path ----

def test_a_primary_ray_with_its_pixels_stream_continues_the_renderers_sample(ctx):
    """The consequence the header states, on the device alone: with a pinhole camera whose rays do not depend on the jitter -- the probe
    camera -- a render's accumulated sums of pixel p are the query's sums for stream p."""
    world, mats, tex = rr.world()
    o, d, llc = rr.ray_set()
    for i in (1, 30):
        ctx.set_scene(hbm_worlds.scene_from_arrays(rr.probe_camera(o[i], llc[i]), world, mats, tex), hbm=True)
        p = m.make_params(rr.N_STREAMS, 1, 4, mode=m.MIRT_MODE_PT, num_bounces=8)
        ctx.accum_reset(p)
        ctx.accum_add(p)
        sums = ctx.accum_read(p).reshape(rr.N_STREAMS, 3)
        got = ctx.trace_radiance(rr.rays_and_streams((i,)), 4)
        assert np.array_equal(got["sum"], sums.astype(np.uint64)), i


# ---- 8. the Layer / Raytracer mirrors ----

def test_raytracer_radiance_returns_the_means():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(32, 16), sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        rays = m.make_radiance_rays((0, 1, 5), [[0, 1, 0], [0, -0.25, -1], [0.5, 0, -1]])
        mean = rt.radiance(rays)                                    # spp = sampling.num_samples_per_pixel
        assert mean.dtype == np.float64 and mean.shape == (3, 3) and np.isfinite(mean).all()
        assert np.abs(mean[0] - [0.5, 0.7, 1.0]).max() < 1e-5      # straight up: the top of the sky's gradient, whatever the stream
        assert np.array_equal(mean, rt.radiance(rays, 4)) and not np.array_equal(mean, rt.radiance(rays, 4, seed=9))
        assert np.array_equal(mean, m.radiance_mean(rt._pick_target().trace_radiance(rays, 4)))
    finally:
        rt.close()
