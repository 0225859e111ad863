"""MIRT_RADIANCE_POOL on the device: radiance_rays_pool_kernel<THREADS,SLOTS,MINW,HOSEK,SORTED>.  The sums are exact
integers, so the pooled schedule must return the bytes of the call without the flag; every case asserts the launch's own name, built
from mirt_bvh_pool_plan, then (i) that the bytes equal those of the same call without the flag and (ii), where the oracle has a claim,
that they equal the CPU oracle's (tests/radiance_ref.py, tests/radiance_frames.py: imported, shared, read-only).  The shapes are the
smallest at which this kernel can go wrong: more items than slots (refill, the queues wrap), fewer items than lanes, units of 1 and 15
rays, waves that run several units, every (slots, waves) geometry with its stacks full, the Hosek blob in front of the pools."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE
import deep_worlds as dw
import feature_ref as fr
import hbm_worlds
import radiance_frames as rf
import radiance_ref as rr
import ray_query_ref as rq
import ray_sort_ref as rs

pytestmark = pytest.mark.gpu

f32 = np.float32
BVH = pytest.mark.parametrize("bvh", ["host", "device"])
ALL = tuple(range(rr.N_RAYS))
SUBSET = rf.SUBSET
FOUR = rr.BOUNCE_RAYS
W, H = fr.W, fr.H                           # 67 x 45 = 3 015 rays: 188 full units and one of 7 rays
DW, DH = rf.DEEP_W, rf.DEEP_H
DEEP_BOUNCES = 6                            # tests/test_gpu_deep_trees.py's
PT = m.MIRT_MODE_PT
POOL, ACC, SORT, FLAT = _abi.MIRT_RADIANCE_POOL, _abi.MIRT_RADIANCE_ACCUMULATE, _abi.MIRT_RADIANCE_SORT, _abi.MIRT_RADIANCE_FLAT
TF = ("false", "true")


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _pool_name(ctx, hosek=False, sort=False, geometry=None):
    """The pooled kernel's name for the resident tree, from mirt_bvh_pool_plan; geometry: the (slots, waves per CU) it must have."""
    depth = ctx.bvh_info()["plan"]["max_depth"]
    plan = m.bvh_pool_plan(depth, hosek)
    assert plan["slots"] != 0 and plan["stack_entries"] == depth
    if geometry is not None:
        assert (plan["slots"], plan["waves_per_cu"]) == geometry, (plan, geometry)
    return "radiance_rays_pool_kernel<%d,%d,4,%s,%s>" % (plan["threads"], plan["slots"], TF[hosek], TF[sort])


def _plain_name(hosek=False, bvh=True, sort=False):
    return f"radiance_rays{'_sorted' if sort else ''}_kernel<{TF[hosek]},{TF[bvh]}>"


def _differ(a, b):
    return np.nonzero((_bytes(a).reshape(-1, 32) != _bytes(b).reshape(-1, 32)).any(1))[0]


def _same(pooled, plain, what):
    assert pooled.dtype == plain.dtype == RADIANCE_DTYPE and pooled.shape == plain.shape
    bad = _differ(pooled, plain)
    print(f"{what}: {len(pooled)} records, {len(bad)} differ between the pooled and the unpooled call")
    assert len(bad) == 0, f"{what}: pooled != unpooled on {len(bad)} of {len(pooled)} records, first {bad[0]}: pooled {pooled[bad[0]]}, unpooled {plain[bad[0]]}"


def _agree(got, want, what):
    bad = _differ(got, want)
    print(f"{what}: {len(got)} records, {len(bad)} differ from the oracle")
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ from the oracle, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _both(ctx, rays, spp, what, hosek=False, geometry=None, **kw):
    """The pooled call's records, after asserting its name and that the call without the flag returns the same bytes."""
    pooled = ctx.trace_radiance(rays, spp, hosek=hosek, pool=True, **kw)
    assert ctx.last_kernel() == _pool_name(ctx, hosek, False, geometry), ctx.last_kernel()
    plain = ctx.trace_radiance(rays, spp, hosek=hosek, **kw)
    assert ctx.last_kernel() == _plain_name(hosek), ctx.last_kernel()
    _same(pooled, plain, what)
    return pooled


def _frame(ctx, cam, w, h, samples, what, hosek=False, geometry=None, **kw):
    """query_frame (the first query overwrites, the later ones accumulate) pooled, name asserted, equal to the unpooled frame."""
    pooled = rf.query_frame(ctx, cam, w, h, samples, hosek=hosek, pool=True, **kw)
    assert ctx.last_kernel() == _pool_name(ctx, hosek, False, geometry), ctx.last_kernel()
    plain = rf.query_frame(ctx, cam, w, h, samples, hosek=hosek, **kw)
    assert ctx.last_kernel() == _plain_name(hosek), ctx.last_kernel()
    _same(pooled, plain, what)
    assert (pooled["samples"] == len(samples)).all() and not pooled["_pad"].any()
    return pooled


def _rendered(ctx, w, h, count, **kw):
    """The device's own accumulation: uint64 [w * h, 3], what mirt_ctx_accum_add gives samples 0 .. count - 1."""
    p = m.make_params(w, h, count, mode=PT, **kw)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    assert ctx.accum_samples() == count
    return ctx.accum_read(p).reshape(-1, 3)


def _set(ctx, bvh="host", sky=None, arr=None):
    world, mats, tex = rr.world()
    ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), world if arr is None else arr, mats, tex, sky),
                  hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _set_fixture(ctx, bvh, sky=None, arr=None):
    ctx.set_scene(rf.fixture_scene_of(fr.fixture().arr if arr is None else arr, 0.0, sky), hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _raw(ctx, rays, n, out, spp, flags, sample_begin=0, num_bounces=8):
    p = _abi.MirtRadianceParams(spp, sample_begin, num_bounces, flags, 0)
    lib = m.lib()
    assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), n, C.byref(p), C.c_void_p(out.ctypes.data)) == 0, lib.mirt_last_error()


# ---- 1. more items than slots, fewer items than lanes: against the oracle ----

@BVH
def test_refill_against_the_oracle(ctx, bvh):
    """256 records = 16 full units at spp 12: 192 items per unit > 112 slots, so slots are refilled and the queues wrap."""
    _set(ctx, bvh)
    rays = rr.rays_and_streams(ALL)
    assert len(rays) == 256 and 16 * 12 > 112 == m.bvh_pool_plan(ctx.bvh_info()["plan"]["max_depth"])["slots"]
    what = f"32 rays x 8 streams at spp 12, {bvh} tree"
    _agree(_both(ctx, rays, 12, what, geometry=(112, 16)), rr.oracle_records(ALL, spp=12), what)
    what = f"sample_begin 5 and a seed at spp 12, {bvh} tree"
    _agree(_both(ctx, rays, 12, what, sample_begin=5, seed=rr.SEED), rr.oracle_records(ALL, spp=12, sample_begin=5, seed=rr.SEED), what)
    _set(ctx, bvh, sky=rr.sky_blob())
    what = f"Hosek sky at spp 12, {bvh} tree"
    got = _both(ctx, rays, 12, what, hosek=True)
    _agree(got, rr.oracle_records(ALL, spp=12, hosek=True), what)
    assert len(_differ(got, rr.oracle_records(ALL, spp=12))) > 0


@BVH
@pytest.mark.parametrize("spp", [1, 7])
def test_under_filled_pools(ctx, bvh, spp):
    """spp 1: 16 items, fewer paths than lanes in every step; spp 7: 112 items = exactly the slots."""
    _set(ctx, bvh)
    what = f"32 rays x 8 streams at spp {spp}, {bvh} tree"
    _agree(_both(ctx, rr.rays_and_streams(ALL), spp, what, geometry=(112, 16)), rr.oracle_records(ALL, spp=spp), what)


# ---- 2. whole frames ----

@BVH
def test_whole_frames_of_the_fixture(ctx, bvh):
    _set_fixture(ctx, bvh)
    what = f"fixture, {bvh} tree, samples 0 1 2"
    got = _frame(ctx, fr.fixture_camera(), W, H, (0, 1, 2), what, geometry=(112, 16))
    _agree(got, rf.frame_records(fr.fixture_scene(), W, H, (0, 1, 2), 8), what)
    assert np.array_equal(got["sum"], _rendered(ctx, W, H, 3, num_bounces=8)), f"{what}: against the device's own accumulation"


# ---- 3. accumulation ----

def test_accumulating_calls_add_up_to_one_call(ctx):
    _set(ctx)
    rays = rr.rays_and_streams(SUBSET)
    whole = _both(ctx, rays, 5, "spp 5")
    _agree(whole, rr.oracle_records(SUBSET, spp=5), "spp 5")
    part = ctx.trace_radiance(rays, 2, pool=True)
    assert (part["samples"] == 2).all()
    back = ctx.trace_radiance(rays, 3, sample_begin=2, into=part, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx)
    assert back is part and np.array_equal(_bytes(part), _bytes(whole)) and (part["samples"] == 5).all()
    dirty = np.zeros(len(rays), RADIANCE_DTYPE)
    _bytes(dirty)[:] = 0xA5
    _raw(ctx, rays, len(rays), dirty, 5, POOL)
    assert ctx.last_kernel() == _pool_name(ctx)
    assert np.array_equal(_bytes(dirty), _bytes(whole)), "without MIRT_RADIANCE_ACCUMULATE the record is overwritten, _pad included"
    _bytes(dirty)[:] = 0xA5
    _raw(ctx, rays, len(rays), dirty, 5, POOL | ACC)
    assert ctx.last_kernel() == _pool_name(ctx)
    assert np.array_equal(dirty["sum"], whole["sum"] + np.uint64(0xA5A5A5A5A5A5A5A5)) and (dirty["samples"] == (0xA5A5A5A5 + 5) % 2 ** 32).all()
    assert not dirty["_pad"].any()
    wrap = np.zeros(len(rays), RADIANCE_DTYPE)
    wrap["samples"] = 0xFFFFFFFE
    _raw(ctx, rays, len(rays), wrap, 5, POOL | ACC)
    assert (wrap["samples"] == 3).all() and np.array_equal(wrap["sum"], whole["sum"]) and not wrap["_pad"].any()      # samples wrap mod 2^32


# ---- 4. ragged units, the record behind the last, waves that run several units ----

def _rays_257():
    rays = np.concatenate([rr.rays_and_streams(ALL), rr.rays_and_streams(ALL[:1])[:1]])
    want = np.concatenate([rr.oracle_records(ALL, spp=9), rr.oracle_records(ALL[:1], spp=9)[:1]])
    return rays, want


def test_ragged_units_and_the_record_behind_the_last(ctx):
    _set(ctx)
    rays, want = _rays_257()
    for n in (1, 15, 16, 17, 63, 64, 65, 257):                         # the last unit holds 1, 15, 16, 1, 15, 16, 1, 1 rays
        out, plain = np.zeros(n + 1, RADIANCE_DTYPE), np.zeros(n + 1, RADIANCE_DTYPE)
        _bytes(out)[:] = 0xA5                                          # the canary: record n must stay as it is
        _bytes(plain)[:] = 0xA5
        _raw(ctx, rays, n, out, 9, POOL)
        assert ctx.last_kernel() == _pool_name(ctx)
        _raw(ctx, rays, n, plain, 9, 0)
        assert ctx.last_kernel() == _plain_name()
        _same(out[:n], plain[:n], f"n_rays {n}")
        _agree(out[:n], want[:n], f"n_rays {n}")
        assert (_bytes(out[n:]) == 0xA5).all(), f"n_rays {n}: the record behind the last was written"
    perm = np.random.default_rng(5).permutation(len(rays))
    _agree(_both(ctx, rays[perm], 9, "a permutation of the batch"), want[perm], "a permutation of the batch")


def test_waves_that_stride_over_several_units(monkeypatch):
    """One block: 17 units on 4 waves, so each wave runs 4 or 5 units and re-initialises its pool and its sums between them."""
    monkeypatch.setenv("MIRT_RADIANCE_POOL_BLOCKS", "1")               # read when a context is created
    rays, want = _rays_257()
    with m.Context(0) as own:
        _set(own)
        what = "257 rays in one block"
        _agree(_both(own, rays, 9, what), want, what)
        _same(own.trace_radiance(rays, 9, pool=True, sort=True), own.trace_radiance(rays, 9), what + ", sorted")
        assert own.last_kernel() == _plain_name()


def test_one_ray_sixteen_streams_and_sixteen_rays_one_stream(ctx):
    """One unit either way: sixteen copies of a ray whose items land on sixteen rows of sums, sixteen rays that share a stream."""
    _set(ctx)
    o, d, _ = rr.ray_set()
    for i in (5, rr.INSIDE_HERO):
        rays = m.make_radiance_rays(np.tile(o[i], (16, 1)), np.tile(d[i], (16, 1)), np.arange(16))
        got = _both(ctx, rays, 4, f"ray {i} x 16 streams")
        _agree(got[:rr.N_STREAMS], rr.oracle_records((i,)), f"ray {i}, streams 0 .. 7")
        if i == 5:                                                  # a diffuse path: the streams differ (the glass hero's do not)
            assert len(np.unique(_bytes(got).reshape(16, 32), axis=0)) > 1
    rays = m.make_radiance_rays(o[:16], d[:16], np.full(16, 3))
    got = _both(ctx, rays, 4, "16 rays, stream 3")
    _agree(got, np.concatenate([rr.oracle_records((i,))[3:4] for i in range(16)]), "16 rays, stream 3")


# ---- 5. high streams ----

@BVH
def test_streams_up_to_0xffffffff_beside_streams_0_to_7(ctx, bvh):
    _set(ctx, bvh)
    high, low = rf.high_stream_rays(SUBSET), rr.rays_and_streams(SUBSET)
    rays = np.stack([high, low], 1).reshape(-1)                     # alternating: every unit mixes high and low streams
    want = np.stack([np.concatenate([rf.high_stream_records(i) for i in SUBSET]), rr.oracle_records(SUBSET)], 1).reshape(-1)
    assert len(rays) == 128 and rays["stream"][0] == 0xFFFFFFF8 and rays["stream"][1] == 0 and rays["stream"][14] == 0xFFFFFFFF
    what = f"streams 0xFFFFFFF8 .. 0xFFFFFFFF beside 0 .. 7, {bvh} tree"
    _agree(_both(ctx, rays, 4, what), want, what)


# ---- 6. bounces, the flat scan ----

def test_bounce_limits_and_where_the_pool_stops(ctx):
    _set(ctx)
    rays = rr.rays_and_streams(ALL)
    for nb in (0, 1, 255):                                          # pooled: the bounce counters are 8 bit
        got = _both(ctx, rays, 4, f"{nb} bounces", num_bounces=nb)
        of_four = got.reshape(rr.N_RAYS, rr.N_STREAMS)[list(FOUR)].reshape(-1)
        _agree(of_four, rr.oracle_records(FOUR, num_bounces=nb), f"{nb} bounces, four rays")
    none = ctx.trace_radiance(rays, 4, num_bounces=0, pool=True)
    assert not none["sum"].any() and (none["samples"] == 4).all() and not none["_pad"].any()
    for nb in (256, 300):                                           # not pooled: the call runs exactly as without the flag
        got = ctx.trace_radiance(rays, 4, num_bounces=nb, pool=True)
        assert ctx.last_kernel() == _plain_name(), ctx.last_kernel()
        _same(got, ctx.trace_radiance(rays, 4, num_bounces=nb), f"{nb} bounces")
        got = ctx.trace_radiance(rays, 4, num_bounces=nb, pool=True, sort=True)
        assert ctx.last_kernel() == _plain_name(sort=True), ctx.last_kernel()
    of_four = got.reshape(rr.N_RAYS, rr.N_STREAMS)[list(FOUR)].reshape(-1)
    _agree(of_four, rr.oracle_records(FOUR, num_bounces=300), "300 bounces, four rays")


def test_the_flat_scan_is_not_pooled(ctx):
    _set(ctx)
    rays = rr.rays_and_streams(SUBSET)
    got = ctx.trace_radiance(rays, 4, flat=True, pool=True)
    assert ctx.last_kernel() == _plain_name(bvh=False), ctx.last_kernel()
    _same(got, ctx.trace_radiance(rays, 4, flat=True), "MIRT_RADIANCE_FLAT | MIRT_RADIANCE_POOL")
    _agree(got, rr.oracle_records(SUBSET), "MIRT_RADIANCE_FLAT | MIRT_RADIANCE_POOL")


# ---- 7. the sorted order ----

@BVH
def test_sorted_and_pooled(ctx, bvh):
    _set_fixture(ctx, bvh)
    cam = fr.fixture_camera()
    perm = rs.permutation(W * H)
    rays = rf.frame_rays(cam, W, H, 0)[perm]
    plain = ctx.trace_radiance(rays, 1)                             # unsorted, unpooled
    assert ctx.last_kernel() == _plain_name()
    got = ctx.trace_radiance(rays, 1, sort=True, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx, sort=True), ctx.last_kernel()
    _same(got, plain, f"the fixture's sample-0 rays shuffled, sorted and pooled, {bvh} tree")
    _agree(got, rf.frame_records(fr.fixture_scene(), W, H, (0,), 8)[perm], "sorted and pooled")
    info = ctx.bvh_info()
    want = rs.order_of(m.ray_sort_codes(info["centre"], info["radius"], rays))
    order = ctx.trace_order()
    assert order.dtype == np.uint32 and np.array_equal(order, want), "the order differs from the stable argsort of the host codes"
    assert not np.array_equal(order, np.arange(len(rays)))
    acc = ctx.trace_radiance(rays, 2, sort=True, pool=True)
    back = ctx.trace_radiance(rays, 3, sample_begin=2, into=acc, sort=True, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx, sort=True) and back is acc
    _same(acc, ctx.trace_radiance(rays, 5), "spp 2 + 3 sorted, pooled and accumulated against spp 5")


# ---- 8. every geometry, stacks full ----

GEOMETRIES = [("line22", "device", "near", 19, (96, 16)), ("stair22", "device", "far", 22, (80, 16)), ("stair25", "device", "far", 25, (64, 16)),
              ("stair28", "device", "far", 28, (112, 12)), ("stair32", "device", "far", 32, (96, 12)), ("line32", "host", "long", 32, (96, 12))]


def _set_deep(ctx, name, builder, view, depth, sky=None):
    cam = rf.deep_cameras(name)[view]
    ctx.set_scene(rf.deep_scene(name, cam, sky), hbm=True, bvh=builder)
    info = ctx.bvh_info()
    assert info["built_on_device"] == (builder == "device") and info["plan"]["max_depth"] == depth, (name, info["plan"])
    assert depth == (dw.DEVICE_DEPTH if builder == "device" else dw.HOST_DEPTH)[name]
    return cam


@pytest.mark.parametrize("name,builder,view,depth,geometry", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_every_geometry_on_deep_trees(ctx, name, builder, view, depth, geometry):
    assert dw.pool_geometry(depth) == geometry
    cam = _set_deep(ctx, name, builder, view, depth)
    what = f"{name} {view}, {builder} tree of depth {depth}, {geometry[0]} slots x {geometry[1]} waves"
    got = _frame(ctx, cam, DW, DH, (0, 1), what, geometry=geometry, num_bounces=DEEP_BOUNCES)
    _agree(got, rf.frame_records(rf.deep_scene(name, cam), DW, DH, (0, 1), DEEP_BOUNCES), what)
    # more items than slots on the sample-0 rays (the oracle has no claim on a jittered frame at spp > 1 from fixed rays)
    _both(ctx, rf.frame_rays(cam, DW, DH, 0), 9, what + ", spp 9", geometry=geometry, num_bounces=DEEP_BOUNCES)


@pytest.mark.parametrize("name,builder,view,depth,geometry", GEOMETRIES[-2:], ids=[g[0] for g in GEOMETRIES[-2:]])
def test_deep_trees_with_the_sky_blob_in_front_of_the_pools(ctx, name, builder, view, depth, geometry):
    cam = _set_deep(ctx, name, builder, view, depth, rr.sky_blob())
    what = f"{name} under the Hosek sky, depth {depth}"
    got = _frame(ctx, cam, DW, DH, (0, 1), what, hosek=True, geometry=geometry, num_bounces=DEEP_BOUNCES)
    _agree(got, rf.frame_records(rf.deep_scene(name, cam, rr.sky_blob()), DW, DH, (0, 1), DEEP_BOUNCES, hosek=True), what)
    _both(ctx, rf.frame_rays(cam, DW, DH, 0), 9, what + ", spp 9", hosek=True, geometry=geometry, num_bounces=DEEP_BOUNCES)


@pytest.mark.parametrize("slots", [80, 64])
def test_forced_geometries_on_a_shallow_tree(monkeypatch, slots):
    monkeypatch.setenv("MIRT_HBM_POOL_SLOTS", str(slots))          # read when a context is created
    with m.Context(0) as own:
        _set_fixture(own, "host")
        assert own.bvh_info()["plan"]["max_depth"] <= 16               # mirt_bvh_pool_plan alone would take 112 slots
        rays = rf.frame_rays(fr.fixture_camera(), W, H, 0)
        for sort in (False, True):
            pooled = own.trace_radiance(rays, 9, pool=True, sort=sort)
            assert own.last_kernel() == f"radiance_rays_pool_kernel<256,{slots},4,false,{TF[sort]}>", own.last_kernel()
            plain = own.trace_radiance(rays, 9)
            assert own.last_kernel() == _plain_name()
            _same(pooled, plain, f"{slots} slots forced on the fixture, sort {sort}")


# ---- 9. the device form ----

def _device_query(ctx, torch, rays, stream, offset=0, preset=0x5A, **kw):
    """trace_radiance_device between torch buffers (4-byte aligned at `offset`) on a caller stream -> the records; the bytes in front
    of the first record and a canary record (and more) behind the last must stay as they were."""
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


def test_device_form_and_worlds_changed_on_the_device(ctx):
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    cam = fr.fixture_camera()
    _set_fixture(ctx, "device")
    rays = rf.frame_rays(cam, W, H, 0)
    host = ctx.trace_radiance(rays, 3)
    got = _device_query(ctx, torch, rays, stream, 4, spp=3, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx, geometry=(112, 16)), ctx.last_kernel()
    _same(got, host, "the device form at a 4-byte offset")
    acc = _device_query(ctx, torch, rays, stream, 4, preset=0, spp=2, sample_begin=1, accumulate=True, pool=True)     # zero records + samples 1, 2
    assert np.array_equal(acc["sum"] + ctx.trace_radiance(rays, 1)["sum"], host["sum"]) and (acc["samples"] == 2).all()
    assert ctx.trace_stats()["kernel_ms"] >= 0.0
    # a refit: same tree, same depth, moved spheres
    moved = rf.moved_fixture_world()
    before = ctx.bvh_info()
    d_moved = torch.from_numpy(_bytes(moved).copy()).to("cuda:0")
    ctx.update_spheres_device(0, len(moved), d_moved.data_ptr())
    assert ctx.bvh_refits() == 1 and ctx.bvh_info()["plan"] == before["plan"]
    got = _device_query(ctx, torch, rays, stream, 4, spp=1, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx, geometry=(112, 16))
    _same(got, ctx.trace_radiance(rays, 1), "after update_spheres_device")
    _agree(got, rf.frame_records(rf.fixture_scene_of(moved), W, H, (0,), 8), "after update_spheres_device")
    assert len(_differ(got, ctx.trace_radiance(rays, 1))) == 0 and len(_differ(host, got)) > 0
    # a world replaced from device memory: a depth-8 tree, then a deeper one -- the geometry and the name follow the new depth
    name = "stair25"
    dcam = rf.deep_cameras(name)["far"]
    arr = dw.ray_set(name)[0]
    mats, tex = hbm_worlds.field_materials()
    copies = hbm_worlds.sphere_array(np.tile([[0.0, 1.0, 0.0]], (1000, 1)), np.full(1000, 1.0), np.zeros(1000))
    ctx.set_scene(hbm_worlds.scene_from_arrays(dcam, copies, mats, tex), hbm=True)
    assert ctx.bvh_info()["plan"]["max_depth"] == 8
    drays = rf.frame_rays(dcam, DW, DH, 0)
    _device_query(ctx, torch, drays, stream, 0, spp=1, pool=True, num_bounces=DEEP_BOUNCES)
    assert ctx.last_kernel() == _pool_name(ctx, geometry=(112, 16))
    d_arr = torch.from_numpy(_bytes(arr).copy()).to("cuda:0")
    ctx.set_spheres_device(len(arr), d_arr.data_ptr())
    assert ctx.bvh_info()["plan"]["max_depth"] == dw.DEVICE_DEPTH[name] == 25
    got = _device_query(ctx, torch, drays, stream, 4, spp=1, pool=True, num_bounces=DEEP_BOUNCES)
    assert ctx.last_kernel() == _pool_name(ctx, geometry=(64, 16)) == "radiance_rays_pool_kernel<256,64,4,false,false>"
    _same(got, ctx.trace_radiance(drays, 1, num_bounces=DEEP_BOUNCES), "after set_spheres_device to a tree of depth 25")
    _agree(got, rf.frame_records(rf.deep_scene(name, dcam), DW, DH, (0,), DEEP_BOUNCES), "after set_spheres_device to a tree of depth 25")


# ---- 10. rays the renderer never makes, degenerate worlds ----

def test_rays_no_camera_makes(ctx):
    """The 1 700 degenerate rays of tests/test_gpu_trace_radiance.py: pooled equals unpooled; the oracle has no claim."""
    _set(ctx)
    o, d, defined = rq.degenerate_rays()                            # zero directions, zero components, NaN and infinite origins, 1e-20, 1e20
    nan_d = np.array([[np.nan, -1, 0], [1, np.inf, 0], [0, -np.inf, np.nan], [np.inf, np.inf, np.inf]], f32)
    o = np.concatenate([o, np.tile(o[:16], (4, 1))])
    d = np.concatenate([d, np.repeat(nan_d, 16, 0)])
    on = np.array([[5, 1, 0], [4, 2, 0], [4, 1, -1], [3, 1, 0], [0.5, 0, 0.5]], f32)
    dirs = np.array([[1, 0.25, 0], [0, 1, 0], [0, 0, 1], [-1, -0.25, 0.5], [0, -1, 0], [0.5, 0, -1]], f32)
    o = np.concatenate([o, np.repeat(on, len(dirs), 0)]).astype(f32)
    d = np.concatenate([d, np.tile(dirs, (len(on), 1))]).astype(f32)
    rays = m.make_radiance_rays(o, d, np.arange(len(o)) % 7)
    assert np.isnan(d).any() and np.isinf(d).any() and np.isnan(o).any() and np.isinf(o).any() and (~(d != 0).any(1)).sum() >= 128
    for nb in (1, 8):
        got = _both(ctx, rays, 2, f"{len(rays)} degenerate rays, {nb} bounces", num_bounces=nb)
        assert (got["samples"] == 2).all()
    _same(ctx.trace_radiance(rays, 2, pool=True, sort=True), got, "degenerate rays, sorted and pooled")
    assert ctx.last_kernel() == _pool_name(ctx, sort=True)


@BVH
@pytest.mark.parametrize("world", list(rf.degenerate_worlds()))
def test_degenerate_worlds(ctx, bvh, world):
    arr = rf.degenerate_worlds()[world]
    ctx.set_scene(rf.degenerate_scene(arr), hbm=True, bvh=bvh)
    what = f"{world}, {bvh} tree"
    got = _frame(ctx, rf.degenerate_camera(), rf.SMALL_W, rf.SMALL_H, (0,), what, geometry=(112, 16))
    _agree(got, rf.frame_records(rf.degenerate_scene(arr), rf.SMALL_W, rf.SMALL_H, (0,), 8), what)
    assert got["sum"].any(1).all()


# ---- 11. refusals and the state a query leaves alone ----

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
    assert both(P(4, 0, 8, POOL, 0)) == (_abi.MIRT_ERR_NO_SCENE,) * 2
    with pytest.raises(m.MirtError) as e:
        ctx.trace_radiance(rays, 4, pool=True)
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    arr, _, _ = rr.world()
    broken = arr.copy()
    broken["material_idx"][7] = 99
    _set(ctx, arr=broken)
    assert both(P(4, 0, 8, POOL, 0)) == (_abi.MIRT_ERR_MATERIAL_INDEX,) * 2
    _set(ctx)
    assert both(P(4, 0, 8, POOL | _abi.MIRT_RADIANCE_SKY_HOSEK, 0)) == (_abi.MIRT_ERR_SKY,) * 2          # no blob in this scene
    for bad in (8, 32, POOL | 8, POOL | 32, POOL | SORT | 32, 1 << 31, 0xFFFFFFF8, 1 << 7):
        assert both(P(4, 0, 8, bad, 0)) == (_abi.MIRT_ERR_BAD_MODE,) * 2, bad
    assert both(P(0, 0, 8, POOL, 0)) == (_abi.MIRT_ERR_SPP_ZERO,) * 2
    assert both(P((1 << 24) + 1, 0, 8, POOL, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    assert both(P(4, 0xFFFFFFFD, 8, POOL, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    for a, b in ((None, po), (pr, None), (None, None)):
        assert both(P(4, 0, 8, POOL, 0), a, b) == (_abi.MIRT_ERR_NULL_POINTER,) * 2
    assert (_bytes(out) == 0xA5).all(), "a refused call writes nothing"
    assert both(P(4, 0, 8, POOL, 0), None, None, 0) == (0, 0) and len(ctx.trace_radiance(rays[:0], 4, pool=True)) == 0        # n_rays == 0
    assert both(P(0, 0, 8, POOL, 0), None, None, 0) == (_abi.MIRT_ERR_SPP_ZERO,) * 2                 # the checks come before "nothing to do"
    assert (_bytes(out) == 0xA5).all()
    # a render, an accumulation -- and a pooled query in between changes neither the statistics nor the sums nor the next render
    p = m.make_params(64, 48, 4, mode=PT, num_bounces=4)
    img = ctx.render(p)
    kernel = ctx.last_kernel()
    ctx.accum_reset(p)
    ctx.accum_add(p)
    sums = ctx.accum_read(p)
    before = ctx.stats()
    assert before["samples"] == 64 * 48 * 4 and before["launches"] >= 2 and before["kernel_ms"] > 0
    got = ctx.trace_radiance(rays, 4, pool=True)
    assert ctx.last_kernel() == _pool_name(ctx) != kernel
    assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p), sums)
    after = ctx.stats()
    assert after["launches"] == 0 and after["kernel_ms_total"] == 0                                       # a query is no render launch
    assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
    assert np.array_equal(ctx.render(p), img)
    _agree(got, rr.oracle_records(SUBSET), "a pooled query between renders")
    st = ctx.trace_stats()
    assert not any(v for k, v in st.items() if k != "kernel_ms")
    ctx.trace_radiance(rays, 4, pool=True)
    st = ctx.trace_stats()
    assert st["kernel_ms"] > 0.0 and not any(v for k, v in st.items() if k != "kernel_ms")


def test_a_nodes_member_answers_as_the_plain_context(ctx):
    _set_fixture(ctx, "host")
    rays = rf.frame_rays(fr.fixture_camera(), W, H, 0)
    want = _both(ctx, rays, 3, "the plain context")
    node = m.Node([0, 0])
    try:
        node.set_scene(fr.fixture_scene(), hbm=True)
        member = node.context(1)
        got = member.trace_radiance(rays, 3, pool=True)
        assert member.last_kernel() == _pool_name(ctx), member.last_kernel()
        _same(got, want, "a node's member")
    finally:
        node.close()


def test_raytracer_radiance_pooled():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(32, 16), sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        rng = np.random.default_rng(1)
        rays = m.make_radiance_rays((0, 1, 5), rng.normal(size=(50, 3)).astype(f32), np.arange(50))
        plain = rt.radiance(rays)
        assert rt._pick_target().last_kernel().startswith("radiance_rays_kernel<")
        pooled = rt.radiance(rays, pool=True)
        assert rt._pick_target().last_kernel().startswith("radiance_rays_pool_kernel<256,112,4,"), rt._pick_target().last_kernel()
        assert pooled.shape == (50, 3) and np.array_equal(pooled, plain)
        assert np.array_equal(rt.radiance(rays, pool=True, sort=True), plain)
    finally:
        rt.close()
    layer = m.Layer.new([32, 16], rp, scene=scene)
    layer.set_global_data()
    try:
        assert np.array_equal(layer.radiance(rays, 2, pool=True), layer.radiance(rays, 2))
    finally:
        layer.close()
