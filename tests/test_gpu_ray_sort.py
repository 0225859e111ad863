"""MIRT_RAYS_SORT and MIRT_RADIANCE_SORT on the device.  A record depends on its ray alone, so a batch traced in the library's order
must give, byte for byte, what the same call gives without the flag -- and, where the existing tests claim one, what the CPU
reference (tests/ray_query_ref.py) or the oracle (tests/radiance_frames.py) gives.  The order itself is held to the stable argsort of
the host codes (mirt_ray_sort_code, which tests/test_ray_sort_abi.py holds to the header's text) under the resident tree's bounds, and
the counting build shows that the kernel runs in the order it reports: on D, whose 3 015 codes are pairwise distinct, the waves of a
sorted launch are the same whatever order D is handed over in, so every counter is.  Every case runs on a host-built and a
device-built tree; every case fails where the flag answers MIRT_ERR_BAD_MODE.  One context for the module.

Measured on an MI355X (what test_counters_show_the_order_that_ran prints; wave_nodes = BVH loop iterations summed over waves, D's
3 015 rays): host-built tree 588 in order, 1 197 shuffled, 605 sorted (either way); device-built tree 584, 1 212, 634.  23 cases in
8 s, 1.6 s of it the context's creation; the slowest case 1.1 s (set A's CPU reference)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE, RAY_HIT_DTYPE
import deep_worlds as dw
import feature_ref as fr
import radiance_frames as rf
import radiance_ref as rr
import ray_query_ref as rq
import ray_sort_ref as rs
from test_gpu_deep_trees import BOUNCES
from test_gpu_deep_trees import _set as _set_deep

pytestmark = pytest.mark.gpu

BVH = pytest.mark.parametrize("bvh", ["host", "device"])
FLAT, ANY, COUNT, SORT = m.MIRT_RAYS_FLAT, m.MIRT_RAYS_ANY_HIT, m.MIRT_RAYS_COUNT, m.MIRT_RAYS_SORT
W, H = fr.W, fr.H
N = rs.N
f32 = np.float32
TF = ("false", "true")


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bytes(got, want, what):
    bad = np.nonzero((_bytes(got).reshape(-1, 32) != _bytes(want).reshape(-1, 32)).any(1))[0]
    assert got.shape == want.shape and len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _set(ctx, arr, bvh):
    ctx.set_scene(rq.scene_of(arr), hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _set_fixture(ctx, bvh, sky=None, aperture=0.0):
    ctx.set_scene(rf.fixture_scene_of(fr.fixture().arr, aperture, sky), hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _host_order(ctx, rays):
    """The stable argsort of the host codes of `rays` under the resident tree's bounds."""
    info = ctx.bvh_info()
    return rs.order_of(m.ray_sort_codes(info["centre"], info["radius"], rays))


def _order_is_right(ctx, rays, what):
    got = ctx.trace_order()
    want = _host_order(ctx, rays)
    assert got.dtype == np.uint32 and np.array_equal(got, want), f"{what}: the order differs from the stable argsort of the host codes at slot {np.nonzero(got != want)[0][:1]}"
    return got


# ---- 1. ray queries ----

@BVH
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sorted_ray_sets_give_the_unsorted_bytes(ctx, name, bvh):
    arr, o, d = rq.SETS[name]()
    _set(ctx, arr, bvh)
    p = rs.permutation(len(o), seed=31)
    rays = rq.rays_of(o[p], d[p])
    ref = rq.set_reference(name)[p]
    for flags in (SORT, SORT | ANY, SORT | FLAT, SORT | COUNT):
        what = f"set {name} permuted, {bvh} tree, flags {flags:#x}"
        got = ctx.trace_rays(rays, flags)
        assert ctx.last_kernel() == f"trace_rays_sorted_kernel<{TF[not flags & FLAT]},{TF[bool(flags & ANY)]},{TF[bool(flags & COUNT)]}>", ctx.last_kernel()
        order = _order_is_right(ctx, rays, what)
        assert not np.array_equal(order, np.arange(len(o)))
        _same_bytes(got, ctx.trace_rays(rays, flags & ~SORT), what)
        assert ctx.last_kernel().startswith("trace_rays_kernel<")
        want = rq.any_hit_of(ref) if flags & ANY else ref
        assert rq.same_bits(got, want).all(), f"{what}: against the CPU reference"
    _same_bytes(ctx.trace_rays(rays, sort=True), ctx.trace_rays(rays), f"set {name}: the wrapper's keyword")
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,false>"


@BVH
def test_sorted_degenerate_rays(ctx, bvh):
    arr, _, _ = rq.set_a()
    _set(ctx, arr, bvh)
    o, d, defined = rq.degenerate_rays()
    p = rs.permutation(len(o), seed=32)
    cen, rad = rq.world_arrays(arr)
    for t_max in (1000.0, np.inf, np.nan):
        rays = rq.rays_of(o[p], d[p], t_max)
        for flags in (SORT, SORT | ANY, SORT | FLAT, SORT | COUNT):
            what = f"degenerate rays, {bvh} tree, t_max {t_max}, flags {flags:#x}"
            got = ctx.trace_rays(rays, flags)
            _order_is_right(ctx, rays, what)
            _same_bytes(got, ctx.trace_rays(rays, flags & ~SORT), what)
        if t_max == t_max:
            want = rq.trace_ref(o[p][defined[p]], d[p][defined[p]], t_max, cen, rad)
            assert rq.same_bits(ctx.trace_rays(rays, SORT)[defined[p]], want).all()


# ---- 2. the order ----

@BVH
def test_the_order_at_every_size_with_a_canary_behind_the_last_hit(ctx, bvh):
    _set_fixture(ctx, bvh)
    o, d = rs.set_d()
    p = rs.permutation(N, seed=33)
    rays = rq.rays_of(o[p], d[p])
    info = ctx.bvh_info()
    assert len(np.unique(m.ray_sort_codes(info["centre"], info["radius"], rays))) == N          # D under this tree's bounds
    full = ctx.trace_rays(rays)
    assert (full["sphere"] != rq.MISS).sum() > 1000
    lib = m.lib()
    for n in rs.SIZES:
        hits = np.zeros(n + 1, RAY_HIT_DTYPE)
        _bytes(hits)[:] = 0xA5
        rc = lib.mirt_ctx_trace_rays(ctx._h, C.c_void_p(rays.ctypes.data), n, SORT, C.c_void_p(hits.ctypes.data))
        assert rc == 0, lib.mirt_last_error()
        assert np.array_equal(_bytes(hits[:n]), _bytes(full[:n])), n
        assert (_bytes(hits[n:]) == 0xA5).all(), f"n = {n}: the record behind the last was written"
        order = np.full(n + 1, 0xA5A5A5A5, np.uint32)
        assert lib.mirt_ctx_trace_order_read(ctx._h, C.c_void_p(order.ctypes.data), n) == 0
        assert np.array_equal(order[:n], _host_order(ctx, rays[:n])) and order[n] == 0xA5A5A5A5, n
        assert np.array_equal(np.sort(order[:n]), np.arange(n))
        if n > 1:
            assert lib.mirt_ctx_trace_order_read(ctx._h, C.c_void_p(order.ctypes.data), n - 1) == _abi.MIRT_ERR_OUT_BUFFER
            assert lib.mirt_ctx_trace_order_read(ctx._h, None, n) == _abi.MIRT_ERR_NULL_POINTER
    # T: all ties -- the index breaks them, the order is the identity
    o, d = rs.set_t()
    rays = rq.rays_of(o, d)
    got = ctx.trace_rays(rays, SORT)
    assert np.array_equal(ctx.trace_order(), np.arange(N))
    _same_bytes(got, ctx.trace_rays(rays), "T")
    assert len(np.unique(_bytes(got).reshape(-1, 32), axis=0)) == 1


def test_no_order_before_the_first_sorted_launch():
    c = m.Context(0)
    try:
        order = np.zeros(4, np.uint32)
        lib = m.lib()
        assert lib.mirt_ctx_trace_order_read(c._h, C.c_void_p(order.ctypes.data), 4) == _abi.MIRT_ERR_NO_SCENE
        c.set_scene(rf.fixture_scene_of(fr.fixture().arr), hbm=True)
        c.trace_rays(rq.rays_of(*rs.set_d()))
        assert lib.mirt_ctx_trace_order_read(c._h, C.c_void_p(order.ctypes.data), 4) == _abi.MIRT_ERR_NO_SCENE
        with pytest.raises(m.MirtError):
            c.trace_order()
        c.trace_rays(rq.rays_of(*rs.set_d())[:3], SORT)
        assert sorted(c.trace_order()) == [0, 1, 2]
    finally:
        c.close()


# ---- 3. counters ----

@BVH
def test_counters_show_the_order_that_ran(ctx, bvh):
    _set_fixture(ctx, bvh)
    o, d = rs.set_d()
    p = rs.permutation(N, seed=34)
    in_order, shuffled = rq.rays_of(o, d), rq.rays_of(o[p], d[p])
    st = {}
    for what, rays, flags in (("in order", in_order, COUNT), ("shuffled", shuffled, COUNT), ("in order, sorted", in_order, SORT | COUNT),
                              ("shuffled, sorted", shuffled, SORT | COUNT)):
        ctx.trace_rays(rays, flags)
        st[what] = {k: v for k, v in ctx.trace_stats().items() if k != "kernel_ms"}
        print(f"D, {bvh} tree, {what}: {st[what]}")
    # the same rays, so the per-lane sums agree everywhere ...
    for what in st:
        for k in ("rays", "hits", "sphere_tests", "roots", "nodes"):
            assert st[what][k] == st["in order"][k], (what, k)
    assert st["in order"]["rays"] == N and 1000 < st["in order"]["hits"] < N
    # ... and the waves of both sorted launches are the same waves: all codes differ, so both run the same rays in the same slots
    assert st["shuffled, sorted"] == st["in order, sorted"]
    assert np.array_equal(p[_host_order(ctx, shuffled)], _host_order(ctx, in_order))
    # not so without the flag (no threshold on how much: DESIGN.md 10.10 records the figures)
    assert st["shuffled"]["wave_nodes"] != st["in order"]["wave_nodes"]
    assert st["shuffled, sorted"]["wave_nodes"] != st["shuffled"]["wave_nodes"]


# ---- 4. radiance ----

def _name(hosek, bvh, sort=True):
    return f"radiance_rays{'_sorted' if sort else ''}_kernel<{TF[hosek]},{TF[bvh]}>"


def _sorted_and_not(ctx, rays, spp, what, hosek=False, **kw):
    """The sorted call's records, after checking its name, its order, and that the call without the flag gives the same bytes."""
    got = ctx.trace_radiance(rays, spp, hosek=hosek, sort=True, **kw)
    assert ctx.last_kernel() == _name(hosek, not kw.get("flat", False)), ctx.last_kernel()
    _order_is_right(ctx, rays, what)
    plain = ctx.trace_radiance(rays, spp, hosek=hosek, **kw)
    assert ctx.last_kernel() == _name(hosek, not kw.get("flat", False), False)
    _same_bytes(got, plain, what)
    return got


@BVH
def test_sorted_frames_of_the_fixture(ctx, bvh):
    cam = fr.fixture_camera()
    rays0 = rf.frame_rays(cam, W, H, 0)
    p = rs.permutation(N, seed=35)
    rays = rays0[p]
    _set_fixture(ctx, bvh)
    want = rf.frame_records(fr.fixture_scene(), W, H, (0,), 8)
    what = f"fixture, sample 0 permuted, {bvh} tree"
    got = _sorted_and_not(ctx, rays, 1, what)
    _same_bytes(got, want[p], what + ", against the oracle")
    _same_bytes(_sorted_and_not(ctx, rays, 1, what + ", flat", flat=True), want[p], what + ", flat, against the oracle")
    # spp 2, then (spp 3 from sample 2) accumulated, is spp 5 -- slot k loads the sums of record order[k]
    five = ctx.trace_radiance(rays, 5)
    acc = ctx.trace_radiance(rays, 2, sort=True)
    _same_bytes(acc, ctx.trace_radiance(rays, 2), what + ", spp 2")
    back = ctx.trace_radiance(rays, 3, sample_begin=2, into=acc, sort=True)
    assert back is acc and ctx.last_kernel() == _name(False, True)
    _same_bytes(acc, five, what + ", 2 + 3 accumulated")
    assert (acc["samples"] == 5).all() and not acc["_pad"].any()
    # a dirty buffer is overwritten without ACCUMULATE
    lib = m.lib()
    dirty = np.zeros(N + 1, RADIANCE_DTYPE)
    _bytes(dirty)[:] = 0xA5
    prm = _abi.MirtRadianceParams(1, 0, 8, _abi.MIRT_RADIANCE_SORT, 0)
    assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), N, C.byref(prm), C.c_void_p(dirty.ctypes.data)) == 0, lib.mirt_last_error()
    _same_bytes(dirty[:N], want[p], what + ", over a dirty buffer")
    assert (_bytes(dirty[N:]) == 0xA5).all()
    # the Hosek build
    _set_fixture(ctx, bvh, sky=rr.sky_blob())
    what = f"fixture under the Hosek sky, sample 0 permuted, {bvh} tree"
    got = _sorted_and_not(ctx, rays, 1, what, hosek=True)
    _same_bytes(got, rf.frame_records(rf.fixture_scene_with_sky(), W, H, (0,), 8, hosek=True)[p], what + ", against the oracle")


@pytest.mark.parametrize("name,view", [("stair32", "far"), ("line32", "long")])
def test_sorted_deep_frames(ctx, name, view):
    """stair32: device-built, all 32 stack entries in use; line32: host-built, the long camera."""
    cam = rf.deep_cameras(name)[view]
    depth = _set_deep(ctx, name, cam)
    assert depth == 32 and ctx.bvh_info()["built_on_device"] == (name in dw.STAIRS)
    n = rf.DEEP_W * rf.DEEP_H
    p = rs.permutation(n, seed=36)
    rays = rf.frame_rays(cam, rf.DEEP_W, rf.DEEP_H, 0)[p]
    what = f"{name} {view}, sample 0 permuted"
    got = _sorted_and_not(ctx, rays, 1, what, num_bounces=BOUNCES)
    _same_bytes(got, ctx.trace_radiance(rays, 1, num_bounces=BOUNCES, flat=True), what + ", against the flat scan")
    _same_bytes(got, rf.frame_records(rf.deep_scene(name, cam), rf.DEEP_W, rf.DEEP_H, (0,), BOUNCES)[p], what + ", against the oracle")


@BVH
def test_sorted_radiance_sizes_with_a_canary_behind_the_last_record(ctx, bvh):
    _set_fixture(ctx, bvh)
    p = rs.permutation(N, seed=37)
    rays = rf.frame_rays(fr.fixture_camera(), W, H, 0)[p]
    full = ctx.trace_radiance(rays[:257], 2)
    lib = m.lib()
    prm = _abi.MirtRadianceParams(2, 0, 8, _abi.MIRT_RADIANCE_SORT, 0)
    for n in (1, 63, 64, 65, 257):
        out = np.zeros(n + 1, RADIANCE_DTYPE)
        _bytes(out)[:] = 0xA5
        assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), n, C.byref(prm), C.c_void_p(out.ctypes.data)) == 0, lib.mirt_last_error()
        assert np.array_equal(_bytes(out[:n]), _bytes(full[:n])), n
        assert (_bytes(out[n:]) == 0xA5).all(), f"n = {n}: the record behind the last was written"
        assert np.array_equal(_order_of_n(ctx, n), _host_order(ctx, rays[:n])), n


def _order_of_n(ctx, n):
    order = np.zeros(n, np.uint32)
    assert m.lib().mirt_ctx_trace_order_read(ctx._h, C.c_void_p(order.ctypes.data), n) == 0
    return order


# ---- 5. scratch and ordering ----

def _device_call(ctx, torch, stream, rays, radiance, offset=4):
    """The sorted device form between torch buffers at a 4-byte offset on a caller stream -> (records' bytes, a closure that checks
    the bytes around them once the stream is done).  Nothing waits here: calls follow each other on the stream."""
    n = len(rays)
    buf = np.zeros(32 * n + 16, np.uint8)
    buf[offset:offset + 32 * n] = _bytes(rays)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(buf).to("cuda:0", non_blocking=False)
        d_out = torch.full((32 * n + 32 + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        if radiance:
            ctx.trace_radiance_device(d_rays.data_ptr() + offset, n, d_out.data_ptr() + offset, 1, sort=True, stream=stream.cuda_stream)
        else:
            ctx.trace_rays_device(d_rays.data_ptr() + offset, n, d_out.data_ptr() + offset, 0, stream=stream.cuda_stream, sort=True)

    def result():
        with torch.cuda.stream(stream):
            out = d_out.cpu().numpy()
        assert (out[:offset] == 0x5A).all() and (out[offset + 32 * n:] == 0x5A).all(), "bytes around the records were written"
        return out[offset:offset + 32 * n].copy(), d_rays
    return result


@BVH
def test_device_form_back_to_back_and_worlds_changed_on_the_device(ctx, bvh):
    import torch
    arr = fr.fixture().arr
    _set_fixture(ctx, bvh)
    stream = torch.cuda.Stream(device="cuda:0")
    p = rs.permutation(N, seed=38)
    rad_rays = rf.frame_rays(fr.fixture_camera(), W, H, 0)[p]
    o, d = rs.set_d()
    ray_rays = rq.rays_of(o[p], d[p])

    def three_calls(what):
        # 257, 65 and 3 015 rays back to back on one stream: the scratch is shared, the stream orders its users
        calls = [(ray_rays[:257], False), (rad_rays[:65], True), (ray_rays, False)]
        pending = [_device_call(ctx, torch, stream, r, radiance) for r, radiance in calls]
        assert ctx.last_kernel() == "trace_rays_sorted_kernel<true,false,false>"
        order = ctx.trace_order()                                       # of the last of them; waits for the device
        assert np.array_equal(order, _host_order(ctx, ray_rays)), what
        for (r, radiance), result in zip(calls, pending):
            got, _ = result()
            want = ctx.trace_radiance(r, 1) if radiance else ctx.trace_rays(r)
            assert np.array_equal(got, _bytes(want)), (what, len(r), radiance)
        return order

    def probes_follow(info, old, what):
        """Probes all over the bounds `info`: here the origin bits decide, and they are those of the resident bounds, not of `old`."""
        rng = np.random.default_rng(39)
        po = (np.asarray(info["centre"], f32) + rng.uniform(-1, 1, (1024, 3)).astype(f32) * f32(info["radius"])).astype(f32)
        probes = rq.rays_of(po, rng.normal(size=(1024, 3)).astype(f32))
        got = ctx.trace_rays(probes, SORT)
        order = _order_is_right(ctx, probes, what)
        assert not np.array_equal(order, rs.order_of(m.ray_sort_codes(old["centre"], old["radius"], probes))), what
        _same_bytes(got, ctx.trace_rays(probes), what)
    first = three_calls("the fixture")
    # every small sphere moved in place from a device tensor, 40 along x (the ground and the heroes stay: the ground is on the
    # always-tested list, outside the tree and its bounds): the bounds move, the order follows the new bvh_info, the bytes the new world
    before = ctx.bvh_info()
    far = rf.moved_fixture_world()
    far["center"][5:, 0] += f32(40.0)
    d_far = torch.from_numpy(_bytes(far[5:]).copy()).to("cuda:0")
    ctx.update_spheres_device(5, len(far) - 5, d_far.data_ptr())
    after = ctx.bvh_info()
    assert ctx.bvh_refits() == 1 and after["centre"][0] - before["centre"][0] > 10
    assert rq.same_bits(ctx.trace_rays(ray_rays, SORT), rq.trace_ref(o[p], d[p], 1000.0, *rq.world_arrays(far))).all()
    three_calls("after update_spheres_device")
    probes_follow(after, before, "probes after update_spheres_device")
    # another sphere table from a device tensor: only a quadrant of the field, so the bounds shrink and the origin bits change
    cen = arr["center"][:, :3]
    corner = arr[(cen[:, 0] > 0) & (cen[:, 2] > 0) & (np.abs(arr["radius"]) < 10)]
    assert 300 < len(corner) < len(arr)
    d_corner = torch.from_numpy(_bytes(corner).copy()).to("cuda:0")
    ctx.set_spheres_device(len(corner), d_corner.data_ptr())
    small = ctx.bvh_info()
    assert small["radius"] < 0.75 * before["radius"] and small["built_on_device"]
    assert rq.same_bits(ctx.trace_rays(ray_rays, SORT), rq.trace_ref(o[p], d[p], 1000.0, *rq.world_arrays(corner))).all()
    third = three_calls("after set_spheres_device")
    assert np.array_equal(np.sort(third), np.arange(N)) and np.array_equal(np.sort(first), np.arange(N))
    probes_follow(small, before, "probes after set_spheres_device")


# ---- 6. errors and state ----

def test_errors_and_untouched_state(ctx):
    lib = m.lib()
    arr, o, d = rq.set_c()
    rays = rq.rays_of(o[:100], d[:100])
    rrays = m.make_radiance_rays(o[:100], d[:100])
    hits = np.zeros(100, RAY_HIT_DTYPE)
    _bytes(hits)[:] = 0xA5
    pr, pq, ph = C.c_void_p(rays.ctypes.data), C.c_void_p(rrays.ctypes.data), C.c_void_p(hits.ctypes.data)
    P = _abi.MirtRadianceParams
    RS = _abi.MIRT_RADIANCE_SORT
    both = lambda p, a=pq, b=ph, k=100: (lib.mirt_ctx_trace_radiance(ctx._h, a, k, C.byref(p), b), lib.mirt_ctx_trace_radiance_device(ctx._h, a, k, C.byref(p), b, None))
    scene, cam = m.scenes.three_spheres()
    lds = m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))
    ctx.set_scene(lds)                                              # an LDS scene: nothing to query, sorted or not
    for flags in (SORT, SORT | COUNT | ANY | FLAT):
        assert lib.mirt_ctx_trace_rays(ctx._h, pr, 100, flags, ph) == _abi.MIRT_ERR_NO_SCENE
        assert lib.mirt_ctx_trace_rays_device(ctx._h, pr, 100, flags, ph, None) == _abi.MIRT_ERR_NO_SCENE
    assert both(P(4, 0, 8, RS, 0)) == (_abi.MIRT_ERR_NO_SCENE,) * 2
    # a sphere whose material does not exist: radiance refuses as a render does, ray queries read no material
    broken = arr.copy()
    broken["material_idx"][7] = 99
    _set(ctx, broken, "host")
    assert both(P(4, 0, 8, RS, 0)) == (_abi.MIRT_ERR_MATERIAL_INDEX,) * 2
    assert lib.mirt_ctx_trace_rays(ctx._h, pr, 100, SORT, ph) == 0
    _bytes(hits)[:] = 0xA5
    _set(ctx, arr, "host")
    for bad in (SORT | 8, SORT | 1 << 31, SORT | 32, 0xFFFFFFF8):
        assert lib.mirt_ctx_trace_rays(ctx._h, pr, 100, bad, ph) == _abi.MIRT_ERR_BAD_MODE
        assert lib.mirt_ctx_trace_rays_device(ctx._h, pr, 100, bad, ph, None) == _abi.MIRT_ERR_BAD_MODE
        assert both(P(4, 0, 8, bad, 0)) == (_abi.MIRT_ERR_BAD_MODE,) * 2
    assert both(P(4, 0, 8, RS | _abi.MIRT_RADIANCE_SKY_HOSEK, 0)) == (_abi.MIRT_ERR_SKY,) * 2
    assert both(P(0, 0, 8, RS, 0)) == (_abi.MIRT_ERR_SPP_ZERO,) * 2
    assert both(P((1 << 24) + 1, 0, 8, RS, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    assert both(P(4, 0xFFFFFFFD, 8, RS, 0)) == (_abi.MIRT_ERR_SPP_RANGE,) * 2
    for a, b in ((None, ph), (pr, None), (None, None)):
        assert lib.mirt_ctx_trace_rays(ctx._h, a, 100, SORT, b) == _abi.MIRT_ERR_NULL_POINTER
        assert lib.mirt_ctx_trace_rays_device(ctx._h, a, 100, SORT, b, None) == _abi.MIRT_ERR_NULL_POINTER
        assert both(P(4, 0, 8, RS, 0), a, b) == (_abi.MIRT_ERR_NULL_POINTER,) * 2
    assert (_bytes(hits) == 0xA5).all(), "a refused call writes nothing"
    # n_rays == 0: MIRT_OK, and the last order stays the last sorted launch's
    ctx.trace_rays(rays[:7], SORT)
    assert lib.mirt_ctx_trace_rays(ctx._h, None, 0, SORT, None) == 0 and lib.mirt_ctx_trace_rays_device(ctx._h, None, 0, SORT | FLAT, None, None) == 0
    assert both(P(4, 0, 8, RS, 0), None, None, 0) == (0, 0) and both(P(0, 0, 8, RS, 0), None, None, 0) == (_abi.MIRT_ERR_SPP_ZERO,) * 2
    assert len(ctx.trace_rays(rays[:0], sort=True)) == 0 and len(ctx.trace_radiance(rrays[:0], 4, sort=True)) == 0
    assert len(ctx.trace_order()) == 7
    # a render, an accumulation -- and sorted queries in between change neither the statistics nor the sums nor the next render
    p = m.make_params(64, 48, 4, mode=m.MIRT_MODE_PT, num_bounces=4)
    img = ctx.render(p)
    kernel = ctx.last_kernel()
    ctx.accum_reset(p)
    ctx.accum_add(p)
    sums = ctx.accum_read(p)
    before = ctx.stats()
    assert before["samples"] == 64 * 48 * 4 and before["launches"] >= 2 and before["kernel_ms"] > 0
    got = ctx.trace_rays(rays, SORT | COUNT)
    assert ctx.last_kernel() == "trace_rays_sorted_kernel<true,false,true>" != kernel
    assert ctx.trace_stats()["rays"] == 100 and ctx.trace_stats()["kernel_ms"] > 0
    rad = ctx.trace_radiance(rrays, 4, sort=True)
    assert ctx.last_kernel() == "radiance_rays_sorted_kernel<false,true>"
    st = ctx.trace_stats()
    assert st["kernel_ms"] > 0.0 and not any(v for k, v in st.items() if k != "kernel_ms")
    assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p), sums)
    after = ctx.stats()
    assert after["launches"] == 0 and after["kernel_ms_total"] == 0
    assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
    assert np.array_equal(ctx.render(p), img)
    assert rq.same_bits(got, rq.set_reference("C")[:100]).all()
    _same_bytes(rad, ctx.trace_radiance(rrays, 4), "a sorted query between renders")
    ctx.set_timing(False)
    ctx.trace_rays(rays, SORT)
    assert ctx.trace_stats()["kernel_ms"] == 0.0                    # kernel_ms follows mirt_ctx_set_timing
    ctx.set_timing(True)
    ctx.trace_radiance(rrays, 1, sort=True)
    assert ctx.trace_stats()["kernel_ms"] > 0.0


def test_raytracer_radiance_sorted():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(32, 16), sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        rng = np.random.default_rng(40)
        rays = m.make_radiance_rays((0, 1, 5), rng.normal(size=(200, 3)))
        mean = rt.radiance(rays, sort=True)
        ctx = rt._pick_target()
        assert ctx.last_kernel().startswith("radiance_rays_sorted_kernel<") and len(ctx.trace_order()) == 200
        assert np.array_equal(mean, rt.radiance(rays)) and ctx.last_kernel().startswith("radiance_rays_kernel<")
        with pytest.raises(ValueError):
            rt.radiance(rays, sort=1)
    finally:
        rt.close()
    layer = m.Layer.new([32, 16], rp, scene=scene)
    layer.set_global_data()
    try:
        assert np.array_equal(layer.radiance(rays, 2, sort=True), layer.radiance(rays, 2))
    finally:
        layer.close()
