"""Every kernel family that walks the BVH of a MIRT_SCENE_HBM scene, on trees 22 to 32 levels deep whose traversal stacks FILL.

The strip kernels keep 32 stack entries per lane, the pooled, ray-query and feature kernels exactly plan.max_depth, and the pooled
kernel picks its geometry from that depth; a push that does not fit is dropped without a trace.  The worlds of tests/deep_worlds.py
make the host builder (the line worlds) and the device builder (the three-axis staircases) produce such trees, and for every tree
read back from the device the numpy walk of tests/bvh_walk_ref.py says how full the stack gets and that one entry fewer would have
changed records -- the audit that lets the byte comparisons below fail.  References: the flat scan restated on the CPU
(ray_query_ref, feature_ref), the flat scan on the device, the LDS builds and the oracle.

Render kernels trace with the fixed bound kMaxT = 1000 and MIN_T = 0.001: a ray sees 20 octaves of distance, a line tree of depth
32 spans 80.  Under the long camera their stacks fill on the line worlds, but what the deepest push guards lies below MIN_T there;
the staircases, seen from 300 extents away, fill the stacks AND are hit where the deepest push decides -- so the staircases are
where a render with a short stack shows, for every pooled geometry; the line worlds add the host builder's depths, real hits at
the dense end and the last entry of the strip kernels' 32."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from bvh_check import check_bvh
from bvh_walk_ref import walk
from helpers import assert_images_equal
from hbm_worlds import c_spheres, field_materials, scene_from_arrays, sphere_array
import deep_worlds as dw
import feature_ref as fr
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 48, 32, 4, 6
PT, POOL, NO_GRID = m.MIRT_MODE_PT, m.MIRT_FLAG_KERNEL_POOL, m.MIRT_FLAG_NO_GRID
FLAT, ANY, COUNT = m.MIRT_RAYS_FLAT, m.MIRT_RAYS_ANY_HIT, m.MIRT_RAYS_COUNT
STRIP = "render_pt_hbm_kernel<false,false,true,true>"
STRIP_FRAME = "render_pt_hbm_frame_kernel<false,false,true,true>"
WORLDS = list(dw.LINES) + list(dw.STAIRS)


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _pt(spp=SPP, **kw):
    kw.setdefault("num_bounces", BOUNCES)
    return m.make_params(W, H, spp, mode=PT, **kw)


def _builder(name):
    return "device" if name in dw.STAIRS else "host"


def _cameras(name):
    """The views a world is rendered from: name -> camera."""
    arr = dw.ray_set(name)[0]
    if name in dw.STAIRS:
        return {"far": dw.staircase_camera(W, H)}
    return {"near": dw.line_camera(W, H), "long": dw.line_camera_long(arr, W, H)}


def _scene(name, cam=None, sky=None):
    arr = dw.ray_set(name)[0]
    mats, tex = field_materials()
    cam = cam if cam is not None else next(iter(_cameras(name).values()))
    return scene_from_arrays(cam, arr, mats, tex, sky)


def _set(ctx, name, cam=None, sky=None):
    """The world on the context, by the builder it is made for; returns the depth of the resident tree, checked."""
    ctx.set_scene(_scene(name, cam, sky), hbm=True, bvh=_builder(name))
    info = ctx.bvh_info()
    assert info["built_on_device"] == (name in dw.STAIRS)
    depth = info["plan"]["max_depth"]
    if name in dw.STAIRS:
        assert depth == dw.DEVICE_DEPTH[name], (name, depth)
    else:
        assert depth == dw.HOST_DEPTH[name] == m.bvh_plan(c_spheres(dw.line(name))[0])["max_depth"]
        assert dw.TARGETS[name][0] <= depth <= dw.TARGETS[name][1]
    assert info["plan"]["n_always"] == 0
    return depth


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _pooled_name(ctx, hosek=False, count=False, frame=False, fast=False):
    plan = m.bvh_pool_plan(ctx.bvh_info()["plan"]["max_depth"], hosek)
    assert plan["slots"] != 0
    tf = ("false", "true")
    return "%srender_pt_pool_hbm%s_kernel<%d,%d,%d,%s,%s>" % ("fast_build::" if fast else "", "_frame" if frame else "", plan["threads"],
                                                              plan["slots"], 1 if count else 4, tf[count], tf[hosek])


def _sums(ctx, p):
    ctx.accum_reset(p)
    ctx.accum_add(p)
    return ctx.accum_read(p)


def _audit(tree, info, name, rays, t_max, device_hits, what):
    """The tree passes check_bvh; with plan.max_depth entries the numpy walk drops no push, returns the device's records and fills
    the stack on >= 16 rays; with one entry fewer >= 16 records change.  Returns (full rays, changed records)."""
    arr = dw.ray_set(name)[0]
    cen, rad = rq.world_arrays(arr)
    count = check_bvh(*tree, info, cen, rad)
    depth = info["plan"]["max_depth"]
    assert count["max_depth"] == depth
    o, d = rays
    got, high, dropped = walk(*tree, info, o, d, t_max, depth, rad)
    full = int((high == depth).sum())
    short, _, dropped1 = walk(*tree, info, o, d, t_max, depth - 1, rad)
    changed = int((~rq.same_bits(short, got)).sum())
    print(f"{what}: depth {depth}, high water {int(high.max())} (on {full} of {len(o)} rays), {int(dropped.sum())} pushes dropped; with "
          f"{depth - 1} entries {int((dropped1 > 0).sum())} rays drop a push and {changed} records change")
    assert rq.same_bits(got, device_hits).all(), f"{what}: the numpy walk and the device disagree on {int((~rq.same_bits(got, device_hits)).sum())} rays"
    assert dropped.sum() == 0 and high.max() == depth and full >= 16
    assert changed >= 16
    return full, changed


# ---- 1. ray queries: trace_rays_kernel with exactly plan.max_depth stack entries ----

@pytest.mark.parametrize("name", WORLDS)
def test_ray_queries_with_full_stacks(ctx, name):
    depth = _set(ctx, name)
    arr, o, d = dw.ray_set(name)
    want = dw.reference(name)
    rays = rq.rays_of(o, d, dw.T_MAX)
    tree = ctx.trace_rays(rays)
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,false>", ctx.last_kernel()
    flat = ctx.trace_rays(rays, FLAT)
    assert ctx.last_kernel() == "trace_rays_kernel<false,false,false>", ctx.last_kernel()
    differ = np.nonzero((_bytes(tree).reshape(-1, 32) != _bytes(flat).reshape(-1, 32)).any(1))[0]
    assert len(differ) == 0, f"{name}: tree != flat on {len(differ)} rays, first {differ[0]}: tree {tree[differ[0]]}, flat {flat[differ[0]]}"
    ok = rq.same_bits(tree, want)
    assert ok.all(), f"{name}: {int((~ok).sum())} rays differ from the CPU reference, first {np.nonzero(~ok)[0][0]}"
    hits = (want["sphere"] != rq.MISS)
    assert 0.2 <= hits.mean() <= 0.95
    # occlusion queries and the counting build
    any_want = rq.any_hit_of(want)
    for flags, kernel in ((ANY, "trace_rays_kernel<true,true,false>"), (ANY | FLAT, "trace_rays_kernel<false,true,false>")):
        got = ctx.trace_rays(rays, flags)
        assert ctx.last_kernel() == kernel, ctx.last_kernel()
        assert np.array_equal(_bytes(got), _bytes(any_want)), f"{name}: any-hit, flags {flags}"
    counted = ctx.trace_rays(rays, COUNT)
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,true>", ctx.last_kernel()
    assert np.array_equal(_bytes(counted), _bytes(tree))
    st = ctx.trace_stats()
    assert st["rays"] == len(rays) and st["hits"] == int(hits.sum()) and st["nodes"] >= len(rays) and st["sphere_tests"] < len(rays) * len(arr)
    _audit(ctx.bvh_read(), ctx.bvh_info(), name, (o, d), dw.T_MAX, tree, f"{name}, {_builder(name)}-built, {depth} levels")


def test_line32_rays_from_device_memory(ctx):
    """A block of trace_rays_kernel takes 32 KB of dynamic LDS at this depth."""
    import torch
    _set(ctx, "line32")
    _, o, d = dw.ray_set("line32")
    rays = rq.rays_of(o, d, dw.T_MAX)
    d_rays = torch.from_numpy(_bytes(rays).copy()).to("cuda:0")
    d_hits = torch.full((32 * len(rays) + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        ctx.trace_rays_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), 0, stream=stream.cuda_stream)
        out = d_hits.cpu().numpy()
    assert (out[32 * len(rays):] == 0x5A).all()
    assert rq.same_bits(out[:32 * len(rays)].copy().view(rq.RAY_HIT_DTYPE), dw.reference("line32")).all()


# ---- 2. feature frames: feature_frame_kernel with exactly plan.max_depth stack entries ----

FEATURE_VIEWS = [("line32", "near"), ("line32", "long"), ("stair32", "far"), ("stair25", "far")]


@pytest.mark.parametrize("name,view", FEATURE_VIEWS)
def test_feature_frames(ctx, name, view):
    cam = _cameras(name)[view]
    depth = _set(ctx, name, cam)
    arr = dw.ray_set(name)[0]
    mats, tex = field_materials()
    ref = fr.FeatureRef(arr, mats, tex, cam, W, H)
    for spp in (0, 2):
        p = m.make_params(W, H, spp, mode=PT)
        tree = ctx.render_features(p)
        assert ctx.last_kernel() == "feature_frame_kernel<true>"
        flat = ctx.render_features(p, flat=True)
        assert ctx.last_kernel() == "feature_frame_kernel<false>"
        assert np.array_equal(_bytes(tree), _bytes(flat)), f"{name} {view} spp {spp}: tree != flat"
        ok = fr.same_bits(tree, ref.of(p))
        assert ok.all(), f"{name} {view} spp {spp}: {int((~ok).sum())} pixels differ from the CPU reference, first {np.argwhere(~ok)[0]}"
    # how full the centre rays make the stack (bound: kMaxT)
    o, d = ref.rays()
    got, high, dropped = walk(*ctx.bvh_read(), ctx.bvh_info(), o, d, 1000.0, depth, rq.world_arrays(arr)[1])
    hits = int((ref.layer()["hits"]["sphere"] != rq.MISS).sum())
    print(f"{name} {view}: {hits} of {W * H} centre rays hit; high water {int(high.max())} of {depth} on {int((high == high.max()).sum())} rays")
    assert rq.same_bits(got, ref.layer()["hits"]).all() and dropped.sum() == 0
    if view != "near":
        assert (high == depth).sum() >= 16
    if view != "long":
        assert hits >= W * H // 10


# ---- 3. render kernels: strip (32 entries) and pooled (plan.max_depth entries, every geometry) ----

def _hosek_sky():
    sky = _abi.MirtSkyState()
    for c in range(3):
        for i, v in enumerate([-1.1, -0.3, 0.5, 1.2, -2.5, 0.4, 0.2, 1.5, 0.6]):
            sky.params[9 * c + i] = v * (1.0 + 0.1 * c)
        sky.radiances[c] = 1.0 + c
    sky.sun_direction[:] = [0.0, 0.6, 0.8, 0.0]
    return sky


@pytest.mark.parametrize("name", WORLDS)
def test_pooled_strip_flat_lds_and_oracle(ctx, oracle, name):
    """Every world under every view: the pooled kernel of the geometry its depth selects, the strip kernel, the flat scan, the LDS
    build and the oracle -- images and exact sums."""
    for view, cam in _cameras(name).items():
        what = f"{name} {view}"
        sd = _scene(name, cam)
        depth = _set(ctx, name, cam)
        plan = m.bvh_pool_plan(depth)
        assert (plan["slots"], plan["waves_per_cu"]) == dw.pool_geometry(depth) and plan["stack_entries"] == depth
        p = _pt()
        strip = ctx.render(p)
        assert ctx.last_kernel() == STRIP, ctx.last_kernel()
        pooled = ctx.render(_pt(flags=POOL))
        assert ctx.last_kernel() == _pooled_name(ctx) and f"<256,{plan['slots']}," in ctx.last_kernel(), ctx.last_kernel()
        print(f"{what}: depth {depth} -> {ctx.last_kernel()} on {plan['waves_per_cu']} waves per CU, {plan['lds_bytes_per_block']} bytes of LDS per block")
        assert_images_equal(pooled, strip, f"{what}: pooled against strip")
        flat = ctx.render(_pt(flags=NO_GRID))
        assert ctx.last_kernel().startswith("render_pt_hbm_kernel<false,false,false,"), ctx.last_kernel()
        assert_images_equal(strip, flat, f"{what}: the tree against the flat scan")
        assert_images_equal(strip, oracle.render(sd, p), f"{what}: against the oracle")
        strip_sums, pooled_sums = _sums(ctx, p), _sums(ctx, _pt(flags=POOL))
        assert ctx.last_kernel() == _pooled_name(ctx)
        assert np.array_equal(pooled_sums, strip_sums), f"{what}: sums, pooled against strip"
        assert np.array_equal(strip_sums, _sums(ctx, _pt(flags=NO_GRID))), f"{what}: sums against the flat scan"
        assert np.array_equal(strip_sums, oracle.render_pt_sums(sd, p)), f"{what}: sums against the oracle"
        ctx.set_scene(sd)                                             # the LDS build of the same scene (these worlds fit LDS)
        assert_images_equal(ctx.render(p), strip, f"{what}: the LDS build against the HBM strip kernel")
        assert np.array_equal(_sums(ctx, p), strip_sums), f"{what}: sums of the LDS build"


# once per geometry, on the staircases (whose primary rays fill the stacks and are decided by the deepest push), and on line32
# under the long view for the strip frame kernel at the edge of its constant
ONCE = list(dw.STAIRS) + ["line32"]


@pytest.mark.parametrize("name", ONCE)
def test_frame_hosek_and_counting_builds_once_per_geometry(ctx, name):
    cam = list(_cameras(name).values())[-1]
    depth = _set(ctx, name, cam)
    p = _pt()
    strip, strip_sums = ctx.render(p), _sums(ctx, p)
    # progressive frames
    frames = []
    for flags, kernel in ((0, STRIP_FRAME), (POOL, _pooled_name(ctx, frame=True))):
        pf = _pt(2, flags=flags)
        ctx.accum_reset(pf)
        imgs = [ctx.accum_frame(pf) for _ in range(2)]
        assert ctx.last_kernel() == kernel, ctx.last_kernel()
        frames.append((imgs, ctx.accum_read(pf)))
    for k in range(2):
        assert_images_equal(frames[1][0][k], frames[0][0][k], f"{name}: frame {k}, pooled against strip")
    assert np.array_equal(frames[0][1], frames[1][1]) and np.array_equal(frames[0][1], strip_sums), f"{name}: 2 x 2 spp in frames"
    assert_images_equal(frames[0][0][1], strip, f"{name}: two frames of 2 spp against one render of 4")
    # the counting builds: a ray's traversal does not depend on the schedule
    cnt = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID
    assert_images_equal(ctx.render(_pt(flags=cnt)), strip, f"{name}: counting strip build")
    assert ctx.last_kernel().startswith("render_pt_hbm_kernel<true,false,true,"), ctx.last_kernel()
    ss = ctx.stats()
    assert_images_equal(ctx.render(_pt(flags=cnt | POOL)), strip, f"{name}: counting pooled build")
    assert ctx.last_kernel() == _pooled_name(ctx, count=True), ctx.last_kernel()
    ps = ctx.stats()
    for k in ("rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses", "lane_iterations", "grid_cells"):
        assert ps[k] == ss[k], (name, k, ps[k], ss[k])
    # the Hosek build
    assert _set(ctx, name, cam, _hosek_sky()) == depth
    hosek = m.MIRT_FLAG_SKY_HOSEK
    want = ctx.render(_pt(flags=hosek))
    assert ctx.last_kernel() == "render_pt_hbm_kernel<false,true,true,true>", ctx.last_kernel()
    got = ctx.render(_pt(flags=hosek | POOL))
    assert ctx.last_kernel() == _pooled_name(ctx, hosek=True), ctx.last_kernel()
    assert_images_equal(got, want, f"{name}: Hosek sky, pooled against strip")
    assert_images_equal(want, ctx.render(_pt(flags=hosek | NO_GRID)), f"{name}: Hosek sky against the flat scan")


def test_every_pooled_geometry_runs(ctx):
    """80, 64 and 96 slots on deep trees and the 12-wave geometry with both of its slot counts, for each builder: the launch's own
    name, world by world."""
    ran = {}
    for name in WORLDS:
        depth = _set(ctx, name)
        ctx.render(_pt(1, flags=POOL))
        kernel = ctx.last_kernel()
        plan = m.bvh_pool_plan(depth)
        assert kernel == "render_pt_pool_hbm_kernel<256,%d,4,false,false>" % plan["slots"], kernel
        ran[name] = (plan["slots"], plan["waves_per_cu"])
    print(ran)
    assert {s for s, _ in ran.values()} == {80, 64, 96, 112} and 12 in {w for _, w in ran.values()}
    for builder in (dw.LINES, dw.STAIRS):
        assert {ran[n] for n in builder} == {(80, 16), (64, 16), (112, 12), (96, 12)}, builder


STACK_EDGE = [("line32", "long")] + [(name, "far") for name in dw.STAIRS]


@pytest.mark.parametrize("name,view", STACK_EDGE)
def test_primary_rays_use_the_last_stack_entry(ctx, name, view):
    """The numpy walk on the renderer's own centre rays (bound kMaxT) of the tree read back: sp reaches plan.max_depth -- on line32
    and stair32 the 32 of the strip kernels' constant -- on >= 16 pixels, and on the staircases a stack one entry short changes the
    records of >= 16 of those very rays (on line32 what the deepest push guards lies below MIN_T: see the module's docstring)."""
    cam = _cameras(name)[view]
    depth = _set(ctx, name, cam)
    arr = dw.ray_set(name)[0]
    rays = np.concatenate([m.camera_pixel_ray(cam, W, H, x, y) for y in range(H) for x in range(W)])
    o, d = rays["origin"].copy(), rays["direction"].copy()
    hits = ctx.trace_rays(rays)
    rad = rq.world_arrays(arr)[1]
    tree, info = ctx.bvh_read(), ctx.bvh_info()
    got, high, dropped = walk(*tree, info, o, d, 1000.0, depth, rad)
    short, _, _ = walk(*tree, info, o, d, 1000.0, depth - 1, rad)
    changed = int((~rq.same_bits(short, got)).sum())
    print(f"{name} {view}: sp reaches {int(high.max())} of {depth} on {int((high == depth).sum())} of {len(o)} centre rays, "
          f"{int((hits['sphere'] != rq.MISS).sum())} of them hit; {depth - 1} entries change {changed} records")
    assert rq.same_bits(got, hits).all() and dropped.sum() == 0 and (high == depth).sum() >= 16
    if name in dw.STAIRS:
        assert changed >= 16
    else:
        assert depth == 32 == m.MIRT_BVH_MAX_DEPTH


def test_fast_math_pooled_against_fast_math_strip(ctx):
    fast = m.MIRT_FLAG_FAST_MATH
    for name in ("line32", "stair32"):
        for view, cam in _cameras(name).items():
            _set(ctx, name, cam)
            strip = ctx.render(_pt(flags=fast))
            assert ctx.last_kernel() == "fast_build::" + STRIP, ctx.last_kernel()
            pooled = ctx.render(_pt(flags=fast | POOL))
            assert ctx.last_kernel() == _pooled_name(ctx, fast=True), ctx.last_kernel()
            assert_images_equal(pooled, strip, f"{name} {view}: fast-math pooled against fast-math strip")


# ---- 4. the depth follows the world ----

def _results(ctx, name):
    """What the three exact-depth kernel families return for the resident world: pooled image, ray records, feature frame."""
    _, o, d = dw.ray_set(name)
    img = ctx.render(_pt(flags=POOL))
    assert ctx.last_kernel() == _pooled_name(ctx), ctx.last_kernel()
    hits = ctx.trace_rays(rq.rays_of(o, d, dw.T_MAX))
    feat = ctx.render_features(m.make_params(W, H, 2, mode=PT))
    return img, _bytes(hits).copy(), _bytes(feat).copy()


@pytest.mark.parametrize("name", ["line32", "stair32"])
def test_the_depth_follows_the_world(ctx, name):
    import torch
    arr = dw.ray_set(name)[0]
    cen, rad = rq.world_arrays(arr)
    cam = list(_cameras(name).values())[-1]                        # the view that fills the stacks
    _set(ctx, name, cam)
    fresh = _results(ctx, name)
    mats, tex = field_materials()
    copies = sphere_array(np.tile([[0.0, 1.0, 0.0]], (1000, 1)), np.full(1000, 1.0), np.zeros(1000))
    d_arr = torch.from_numpy(_bytes(arr).copy()).to("cuda:0")
    depths = []
    for how in ("set_spheres", "set_spheres_device"):
        ctx.set_scene(scene_from_arrays(cam, copies, mats, tex), hbm=True)
        assert ctx.bvh_info()["plan"]["max_depth"] == 8                # ceil(log2(1000 / 4))
        if how == "set_spheres":
            ctx.set_spheres(arr)
        else:
            ctx.set_spheres_device(len(arr), d_arr.data_ptr())
        info = ctx.bvh_info()
        count = check_bvh(*ctx.bvh_read(), info, cen, rad)
        assert info["built_on_device"] and count["max_depth"] == info["plan"]["max_depth"]
        depths.append(info["plan"]["max_depth"])
        assert depths[-1] == dw.DEVICE_DEPTH[name]                   # set_spheres* builds on the device
        got = _results(ctx, name)
        assert_images_equal(got[0], fresh[0], f"{name}: pooled image after {how}")
        assert np.array_equal(got[1], fresh[1]) and np.array_equal(got[2], fresh[2]), f"{name}: rays / features after {how}"
    print(f"{name}: depth {depths} after set_spheres / set_spheres_device over a tree of depth 8")
    assert depths[0] == depths[1] == dw.DEVICE_DEPTH[name] > 8
    before = [a.tobytes() for a in ctx.bvh_read()]
    ctx.update_spheres(0, arr)
    assert ctx.bvh_info()["plan"]["max_depth"] == depths[1] and [a.tobytes() for a in ctx.bvh_read()] == before
    got = _results(ctx, name)
    assert_images_equal(got[0], fresh[0], f"{name}: pooled image after update_spheres")
    assert np.array_equal(got[1], fresh[1]) and np.array_equal(got[2], fresh[2])


@pytest.mark.parametrize("name", WORLDS)
def test_the_other_builders_tree_of_every_world(ctx, name):
    """Each world through the builder it was NOT made for: a valid tree of the recorded depth, and the same ray records."""
    other = "host" if name in dw.STAIRS else "device"
    arr, o, d = dw.ray_set(name)
    ctx.set_scene(_scene(name), hbm=True, bvh=other)
    info = ctx.bvh_info()
    count = check_bvh(*ctx.bvh_read(), info, *rq.world_arrays(arr))
    want = (dw.HOST_DEPTH if other == "host" else dw.DEVICE_DEPTH)[name]
    print(f"{name}: {other}-built depth {count['max_depth']}")
    assert info["built_on_device"] == (other == "device") and count["max_depth"] == info["plan"]["max_depth"] == want
    assert rq.same_bits(ctx.trace_rays(rq.rays_of(o, d, dw.T_MAX)), dw.reference(name)).all()


def test_a_node_sizes_its_members_stacks(ctx):
    for name in ("line26", "stair28"):
        cam = list(_cameras(name).values())[-1]
        _set(ctx, name, cam)
        want = ctx.render(_pt(flags=POOL))
        assert ctx.last_kernel() == _pooled_name(ctx)
        node = m.Node([0, 0])
        try:
            node.set_scene(_scene(name, cam), hbm=True, bvh=_builder(name))
            assert_images_equal(node.render(_pt(flags=POOL)), want, f"{name}: node of 2, pooled")
            assert node.context(0).bvh_info()["plan"] == ctx.bvh_info()["plan"]
            assert node.context(0).last_kernel() == _pooled_name(ctx), node.context(0).last_kernel()
        finally:
            node.close()


# ---- 5. forced geometries on a shallow tree: "the build is wrong" apart from "deep trees are wrong" ----

@pytest.mark.parametrize("slots", [80, 64])
def test_forced_geometries_on_a_shallow_tree(monkeypatch, slots):
    from hbm_worlds import look, rtiow_field
    monkeypatch.setenv("MIRT_HBM_POOL_SLOTS", str(slots))          # read when a context is created
    arr, mats, tex = rtiow_field(3000)
    with m.Context(0) as own:
        own.set_scene(scene_from_arrays(look(W, H, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex), hbm=True)
        assert own.bvh_info()["plan"]["max_depth"] <= 16               # mirt_bvh_pool_plan alone would take 112 slots
        strip = own.render(_pt())
        assert own.last_kernel() == STRIP
        pooled = own.render(_pt(flags=POOL))
        assert own.last_kernel() == f"render_pt_pool_hbm_kernel<256,{slots},4,false,false>", own.last_kernel()
        assert_images_equal(pooled, strip, f"{slots} slots forced on rtiow_field(3000)")
