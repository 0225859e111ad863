"""mirt_ctx_trace_rays* on the device: the BVH walk (nearest_hit_bvh itself) and the flat scan against the exact CPU restatement of
the flat scan (tests/ray_query_ref.py), ray by ray and bit by bit, on inputs no camera produces.  One context for the module; the
references of the ray sets are computed once (ray_query_ref caches them)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RAY_DTYPE, RAY_HIT_DTYPE
import hbm_worlds
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

FLAT, ANY, COUNT = m.MIRT_RAYS_FLAT, m.MIRT_RAYS_ANY_HIT, m.MIRT_RAYS_COUNT
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _set(ctx, arr, bvh="host"):
    ctx.set_scene(rq.scene_of(arr), hbm=True, bvh=bvh)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _agree(got, want, what):
    """Every record of `got` has the reference's bits (a NaN for a NaN); the message names the first ray that differs."""
    ok = rq.same_bits(got, want)
    bad = np.nonzero(~ok)[0]
    print(f"{what}: {len(got)} rays, {int((want['sphere'] != rq.MISS).sum())} reference hits, {len(bad)} records differ")
    assert ok.all(), f"{what}: {len(bad)} of {len(got)} rays differ, first ray {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _tree_and_flat(ctx, rays, what, flags=0):
    """The tree's records, after checking that the flat scan on the device returns the same bytes."""
    tree = ctx.trace_rays(rays, flags)
    flat = ctx.trace_rays(rays, flags | FLAT)
    differ = np.nonzero((_bytes(tree).reshape(-1, 32) != _bytes(flat).reshape(-1, 32)).any(1))[0]
    print(f"{what}: tree and flat differ in {len(differ)} of {len(rays)} records")
    assert len(differ) == 0, f"{what}: tree != flat at ray {differ[0]}: {rays[differ[0]]} -> tree {tree[differ[0]]}, flat {flat[differ[0]]}"
    return tree


# ---- 1. the three ray sets, host-built and device-built tree ----

@pytest.mark.parametrize("bvh", ["host", "device"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_ray_sets_match_the_cpu_reference(ctx, name, bvh):
    arr, o, d = rq.SETS[name]()
    _set(ctx, arr, bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")
    got = _tree_and_flat(ctx, rq.rays_of(o, d), f"set {name}, {bvh} tree")
    _agree(got, rq.set_reference(name), f"set {name}, {bvh} tree")
    assert ctx.last_kernel() == "trace_rays_kernel<false,false,false>"


# ---- 2. per-ray bounds ----

def test_t_max_bounds_every_ray_strictly(ctx):
    arr, o, d = rq.set_a()
    _set(ctx, arr)
    ref = rq.set_reference("A")
    t = np.where(ref["sphere"] != rq.MISS, ref["t"], f32(10.0)).astype(f32)
    bounds = {"1000": np.full(len(o), 1000.0, f32), "half": (t * f32(0.5)).astype(f32), "next up": np.nextafter(t, f32(np.inf)), "t itself": t,
              "next down": np.nextafter(t, f32(0.0)), "inf": np.full(len(o), np.inf, f32), "nan": np.full(len(o), np.nan, f32),
              "0": np.zeros(len(o), f32), "-1": np.full(len(o), -1.0, f32), "-inf": np.full(len(o), -np.inf, f32)}
    hit = ref["sphere"] != rq.MISS
    for what, t_max in bounds.items():
        got = _tree_and_flat(ctx, rq.rays_of(o, d, t_max), f"t_max = {what}")
        want = rq.set_reference("A", t_max)
        _agree(got, want, f"t_max = {what}")
        if what in ("1000", "next up", "inf"):
            assert np.array_equal(got["sphere"], ref["sphere"])
        if what in ("t itself", "next down"):                   # strict: the winner at t does not win with t_max = t
            assert (got["sphere"][hit] != ref["sphere"][hit]).all() and ((got["t"][hit] < t[hit]) | (got["sphere"][hit] == rq.MISS)).all()
        if what in ("nan", "0", "-1", "-inf"):
            assert (got["sphere"] == rq.MISS).all() and not _bytes(got).reshape(-1, 8, 4)[:, [0, 2, 3, 4, 5, 6, 7]].any()


# ---- 3. rays no camera produces ----

def test_degenerate_rays(ctx):
    arr, _, _ = rq.set_a()
    _set(ctx, arr)
    o, d, defined = rq.degenerate_rays()
    cen, rad = rq.world_arrays(arr)
    for t_max in (1000.0, np.inf):
        got = _tree_and_flat(ctx, rq.rays_of(o, d, t_max), f"degenerate rays, t_max {t_max}")
        want = rq.trace_ref(o[defined], d[defined], t_max, cen, rad)
        _agree(got[defined], want, f"degenerate rays with finite inputs, t_max {t_max}")
        zero = ~(d != 0).any(1)
        assert zero.sum() >= 128 and (got["sphere"][zero] == rq.MISS).all()              # a zero direction is a defined miss
        assert (got["sphere"][~np.isfinite(o).all(1)] == rq.MISS).all()                  # so is a non-finite origin
    assert (want["sphere"] != rq.MISS).sum() >= 300                                      # the finite ones do hit the field


# ---- 4. other adversarial worlds ----

def _aimed_rays(seed, n, eye, at, spread, eye_spread=0.0):
    rng = np.random.default_rng(seed)
    o = np.asarray(eye, np.float64) + rng.uniform(-eye_spread, eye_spread, (n, 3))
    d = np.asarray(at, np.float64) + rng.uniform(-spread, spread, (n, 3)) - o
    d *= rng.uniform(0.25, 4.0, n)[:, None]
    return o.astype(f32), d.astype(f32)


def _world_case(name):
    if name in ("copies", "inside"):
        arr = rq.adversarial(name)
        o, d = _aimed_rays(11, 384, (0, 0, 1), (0, 0, -3), 1.0) if name == "copies" else _aimed_rays(12, 384, (0.1, 0.2, 0.3), (0, 0, 0), 4.0, eye_spread=2.0)
    elif name == "identical 10000":
        arr = hbm_worlds.sphere_array(np.tile([[1.0, 0.5, -4.0]], (10000, 1)), np.full(10000, 0.8), np.arange(10000) % 5)
        o, d = _aimed_rays(13, 256, (0, 0, 2), (1.0, 0.5, -4.0), 1.2)
    else:
        arr = hbm_worlds.sphere_array([[0.5, -0.25, -5.0]], [1.25], [1])
        o, d = _aimed_rays(14, 256, (0, 0, 2), (0.5, -0.25, -5.0), 2.0)
    return arr, o, d


@pytest.mark.parametrize("bvh", ["host", "device"])
@pytest.mark.parametrize("name", ["copies", "inside", "identical 10000", "single"])
def test_adversarial_worlds(ctx, name, bvh):
    arr, o, d = _world_case(name)
    _set(ctx, arr, bvh)
    plan = ctx.bvh_info()["plan"]
    if name == "identical 10000":
        assert plan["max_depth"] >= 12                                # the median tree: nothing else separates equal centres
    if name == "single":
        assert plan["n_nodes"] == 0                                   # the root is a leaf
    got = _tree_and_flat(ctx, rq.rays_of(o, d), f"{name}, {bvh} tree")
    want = rq.trace_ref(o, d, 1000.0, *rq.world_arrays(arr))
    _agree(got, want, f"{name}, {bvh} tree")
    hits = got["sphere"] != rq.MISS
    assert 0.2 <= hits.mean() and (name == "inside" or hits.mean() <= 0.95)          # hits and misses both occur
    if name in ("copies", "identical 10000"):
        assert (got["sphere"][hits] == 0).all()                       # the lowest index wins among equals


def test_the_empty_world_misses_everything(ctx):
    arr, o, d = _world_case("single")
    _set(ctx, arr)
    ctx.set_spheres(arr[:0])
    for flags in (0, ANY, COUNT):
        got = _tree_and_flat(ctx, rq.rays_of(o, d), "empty world", flags)
        assert (got["sphere"] == rq.MISS).all() and rq.same_bits(got, rq.any_hit_of(got)).all()
    st = ctx.trace_stats()
    assert st["rays"] == len(o) and st["sphere_tests"] == 0 and st["hits"] == 0


# ---- 5. occlusion queries ----

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_any_hit_is_nearest_hit_or_miss(ctx, name):
    arr, o, d = rq.SETS[name]()
    _set(ctx, arr)
    ref = rq.set_reference(name)
    rng = np.random.default_rng(21)
    factor = rng.choice(np.array([0.5, 0.999, 1.0, 1.001, 2.0], f32), len(o))
    bounded = np.where(ref["sphere"] != rq.MISS, ref["t"] * factor, f32(1000.0)).astype(f32)
    for what, t_max in (("t_max 1000", 1000.0), ("per-ray t_max", bounded)):
        want = rq.any_hit_of(rq.set_reference(name, t_max))
        got = _tree_and_flat(ctx, rq.rays_of(o, d, t_max), f"any-hit, set {name}, {what}", ANY)
        assert np.array_equal(_bytes(got), _bytes(want)), f"any-hit, set {name}, {what}: {int((got['sphere'] != want['sphere']).sum())} flags differ"
        assert 0 < (want["sphere"] == 0).sum() < len(o)
    assert ctx.last_kernel() == "trace_rays_kernel<false,true,false>"


# ---- 6. the counting build ----

def test_counting_build(ctx):
    arr, o, d = rq.set_a()
    _set(ctx, arr)
    rays, ref = rq.rays_of(o, d), rq.set_reference("A")
    n, n_hits = len(rays), int((ref["sphere"] != rq.MISS).sum())
    st = {}
    for what, flags in (("tree", 0), ("flat", FLAT), ("tree any", ANY), ("flat any", FLAT | ANY)):
        plain = ctx.trace_rays(rays, flags)
        assert not any(v for k, v in ctx.trace_stats().items() if k != "kernel_ms"), "no counters without MIRT_RAYS_COUNT"
        counted = ctx.trace_rays(rays, flags | COUNT)
        assert np.array_equal(_bytes(plain), _bytes(counted)), what
        st[what] = ctx.trace_stats()
        print(what, st[what])
        assert st[what]["rays"] == n and st[what]["hits"] == n_hits and st[what]["kernel_ms"] > 0
    assert ctx.last_kernel() == "trace_rays_kernel<false,true,true>"
    assert st["flat"]["sphere_tests"] == n * len(arr) and st["flat"]["nodes"] == 0 and st["flat"]["wave_nodes"] == 0
    assert st["tree"]["sphere_tests"] < st["flat"]["sphere_tests"]
    assert st["tree"]["nodes"] >= n and n // 64 <= st["tree"]["wave_nodes"] <= st["tree"]["nodes"]
    assert st["tree any"]["sphere_tests"] <= st["tree"]["sphere_tests"] and st["tree any"]["nodes"] <= st["tree"]["nodes"]
    assert st["flat any"]["sphere_tests"] <= st["flat"]["sphere_tests"]
    assert st["tree"]["roots"] >= n_hits and st["flat"]["roots"] >= st["tree"]["roots"]


# ---- 7. sizes: whole waves, tails, more than one block ----

@pytest.mark.parametrize("flags", [0, FLAT], ids=["tree", "flat"])
def test_sizes_and_the_record_behind_the_last(ctx, flags):
    arr, o, d = rq.set_a()
    _set(ctx, arr)
    rays = rq.rays_of(np.concatenate([o, o[:1]]), np.concatenate([d, d[:1]]))          # 4097 rays
    full = ctx.trace_rays(rays, flags)
    assert rq.same_bits(full[:4096], rq.set_reference("A")).all()
    lib = m.lib()
    for n in (1, 63, 64, 65, 257, 4097):
        hits = np.zeros(n + 1, RAY_HIT_DTYPE)
        _bytes(hits)[:] = 0xA5                                      # the canary: record n must stay as it is
        rc = lib.mirt_ctx_trace_rays(ctx._h, C.c_void_p(rays.ctypes.data), n, flags, C.c_void_p(hits.ctypes.data))
        assert rc == 0, lib.mirt_last_error()
        assert np.array_equal(_bytes(hits[:n]), _bytes(full[:n])), n
        assert (_bytes(hits[n:]) == 0xA5).all(), f"n = {n}: the record behind the last was written"


# ---- 8. the device path ----

def _device_trace(ctx, torch, rays, flags, stream, offset=0):
    """trace_rays_device between torch buffers (4-byte aligned at `offset`) on a caller stream -> the hit records."""
    n = len(rays)
    buf = np.zeros(32 * n + 16, np.uint8)
    buf[offset:offset + 32 * n] = _bytes(rays)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(buf).to("cuda:0", non_blocking=False)
        d_hits = torch.full((32 * n + 32 + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        ctx.trace_rays_device(d_rays.data_ptr() + offset, n, d_hits.data_ptr() + offset, flags, stream=stream.cuda_stream)
        out = d_hits.cpu().numpy()                                  # ordered after the trace on the same stream
    assert (out[:offset] == 0x5A).all() and (out[offset + 32 * n:] == 0x5A).all(), "bytes around the hit records were written"
    return out[offset:offset + 32 * n].copy().view(RAY_HIT_DTYPE)


def test_device_path_and_worlds_changed_on_the_device(ctx):
    import torch
    arr, o, d = rq.set_a()
    o, d = o[:1500], d[:1500]
    _set(ctx, arr, "device")
    rays = rq.rays_of(o, d)
    host = ctx.trace_rays(rays)
    stream = torch.cuda.Stream(device="cuda:0")
    for flags in (0, FLAT, ANY):
        for offset in (0, 4):
            got = _device_trace(ctx, torch, rays, flags, stream, offset)
            assert np.array_equal(_bytes(got), _bytes(ctx.trace_rays(rays, flags))), (flags, offset)
    # spheres moved from a device tensor: the refitted tree answers for the moved world
    rng = np.random.default_rng(8)
    moved = arr.copy()
    first, count = 700, 900
    moved["center"][first:first + count, :3] += rng.normal(0, 1.5, (count, 3)).astype(f32)
    moved["radius"][first:first + count] *= rng.uniform(0.5, 3.0, count).astype(f32)
    d_moved = torch.from_numpy(_bytes(moved[first:first + count]).copy()).to("cuda:0")
    ctx.update_spheres_device(first, count, d_moved.data_ptr())
    assert ctx.bvh_refits() == 1
    want = rq.trace_ref(o, d, 1000.0, *rq.world_arrays(moved))
    got = _tree_and_flat(ctx, rays, "after update_spheres_device")
    _agree(got, want, "after update_spheres_device")
    assert not np.array_equal(_bytes(got), _bytes(host)), "the move changes answers"
    assert np.array_equal(_bytes(_device_trace(ctx, torch, rays, 0, stream)), _bytes(got))
    # another count, from a device tensor
    fewer = np.concatenate([moved[:5], moved[1200:2600]])
    d_fewer = torch.from_numpy(_bytes(fewer).copy()).to("cuda:0")
    ctx.set_spheres_device(len(fewer), d_fewer.data_ptr())
    want = rq.trace_ref(o, d, 1000.0, *rq.world_arrays(fewer))
    got2 = _tree_and_flat(ctx, rays, "after set_spheres_device")
    _agree(got2, want, "after set_spheres_device")
    assert np.array_equal(_bytes(_device_trace(ctx, torch, rays, 0, stream, 4)), _bytes(got2))
    for world, was in ((moved, got), (fewer, got2)):                # a fresh scene of the same world answers the same
        _set(ctx, world, "host")
        assert np.array_equal(_bytes(ctx.trace_rays(rays)), _bytes(was))


# ---- 9. errors, and what a trace leaves alone ----

def test_errors_and_untouched_state(ctx):
    lib = m.lib()
    arr, o, d = rq.set_c()
    rays = rq.rays_of(o[:100], d[:100])
    hits = np.zeros(100, RAY_HIT_DTYPE)
    pr, ph = C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data)
    scene, cam = m.scenes.three_spheres()
    lds = m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))
    ctx.set_scene(lds)                                              # an LDS scene: nothing to query
    for fn, args in ((lib.mirt_ctx_trace_rays, (pr, 100, 0, ph)), (lib.mirt_ctx_trace_rays_device, (pr, 100, 0, ph, None))):
        assert fn(ctx._h, *args) == _abi.MIRT_ERR_NO_SCENE and b"MIRT_SCENE_HBM" in lib.mirt_last_error()
    with pytest.raises(m.MirtError) as e:
        ctx.trace_rays(rays)
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    _set(ctx, arr)
    for bad in (8, 1 << 31, 0xFFFFFFF8):
        assert lib.mirt_ctx_trace_rays(ctx._h, pr, 100, bad, ph) == _abi.MIRT_ERR_BAD_MODE
        assert lib.mirt_ctx_trace_rays_device(ctx._h, pr, 100, bad, ph, None) == _abi.MIRT_ERR_BAD_MODE
    for a, b in ((None, ph), (pr, None), (None, None)):
        assert lib.mirt_ctx_trace_rays(ctx._h, a, 100, 0, b) == _abi.MIRT_ERR_NULL_POINTER
        assert lib.mirt_ctx_trace_rays_device(ctx._h, a, 100, 0, b, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_trace_stats(ctx._h, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_trace_rays(ctx._h, None, 0, 0, None) == 0 and lib.mirt_ctx_trace_rays_device(ctx._h, None, 0, FLAT, None, None) == 0
    assert len(ctx.trace_rays(rays[:0])) == 0
    # a render, an accumulation -- and a trace in between changes neither the statistics nor the sums
    p = m.make_params(64, 48, 4, mode=m.MIRT_MODE_PT, num_bounces=4)
    img = ctx.render(p)
    kernel = ctx.last_kernel()
    ctx.accum_reset(p)
    ctx.accum_add(p)
    sums = ctx.accum_read(p)
    before = ctx.stats()                                            # of the add; launches are counted from here on
    assert before["samples"] == 64 * 48 * 4 and before["launches"] >= 2 and before["kernel_ms"] > 0
    got = ctx.trace_rays(rays, COUNT)
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,true>" != kernel
    assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p), sums)
    after = ctx.stats()
    assert after["launches"] == 0 and after["kernel_ms_total"] == 0                                       # a trace is no render launch
    assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
    assert ctx.trace_stats()["rays"] == 100
    assert np.array_equal(ctx.render(p), img)
    _agree(got, rq.set_reference("C")[:100], "a trace between renders")
    ctx.set_timing(False)
    ctx.trace_rays(rays)
    assert ctx.trace_stats()["kernel_ms"] == 0.0                    # kernel_ms follows mirt_ctx_set_timing
    ctx.set_timing(True)
    ctx.trace_rays(rays)
    assert ctx.trace_stats()["kernel_ms"] > 0.0


# ---- 10. picking ----

def _pixel_of(cam, w, h, point):
    """The pixel onto which `point` projects: solve eye + k (llc + u hor + v ver - eye) = point for (u, v)."""
    eye, hor, ver, llc = (np.asarray(a[:3], np.float64) for a in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    u, v, _ = np.linalg.solve(np.stack([hor, ver, -(np.asarray(point, np.float64) - eye)], 1), eye - llc)
    return int(u * w), int((1.0 - v) * h)


def test_layer_pick():
    scene, cam = m.scenes.three_spheres()
    w, h = 160, 96
    rp = m.RenderParams(camera=cam, viewport_size=(w, h))
    layer = m.Layer.new([w, h], rp, scene=scene)
    layer.set_global_data()
    try:
        gpu_cam = layer.camera.c
        seen = {}
        for i, s in enumerate(scene.spheres[1:], start=1):          # the two unit spheres; the ground's centre lies below the frame
            x, y = _pixel_of(gpu_cam, w, h, s.center)
            assert 0 <= x < w and 0 <= y < h
            hit = layer.pick(x, y)
            assert hit is not None and hit["sphere"] == i, (i, x, y, hit)
            assert abs(float(np.linalg.norm(hit["point"] - np.asarray(s.center, f32))) - 1.0) < 1e-4 and hit["t"] > 0.001
            seen[i] = (x, y)
        assert layer._hbm and layer._ctx.last_kernel() == "trace_rays_kernel<true,false,false>"
        assert layer.pick(w // 2, 0) is None                        # the sky above the horizon
        ground = layer.pick(w // 2, h - 1)
        assert ground is not None and ground["sphere"] == 0
        layer.set_data(rp)                                          # the layer still renders, and picks afterwards
        assert layer.register_texture().shape == (h, w, 4)
        x, y = seen[1]
        assert layer.pick(x, y)["sphere"] == 1
        rt = m.Raytracer(scene, rp)
        try:
            assert rt.pick(x, y)["sphere"] == 1 and rt.pick(w // 2, 0) is None
        finally:
            rt.close()
        with pytest.raises(ValueError):
            layer.pick(w, 0)
    finally:
        layer.close()
