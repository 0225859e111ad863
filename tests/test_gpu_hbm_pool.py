"""MIRT_FLAG_KERNEL_POOL on a MIRT_SCENE_HBM scene: render_pt_pool_hbm_kernel, the pooled schedule with BVH traversal.

A schedule changes the ORDER in which a frame's paths are served, never a path: every check here is byte-equal images (and equal
exact 64-bit sums where sums are read) against the same context rendering without the flag, with the kernel's name asserted on
both sides; the LDS builds, the flat scan and the oracle are further witnesses."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from bvh_check import always_list
from helpers import assert_images_equal, scene_data
from hbm_worlds import field_materials, look, rtiow_field, scene_from_arrays, sphere_array
from test_gpu_hbm_scene import _adversarial, _lds_scenes

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
POOL = m.MIRT_FLAG_KERNEL_POOL
STRIP = "render_pt_hbm_kernel<false,false,true,true>"
POOLED = "render_pt_pool_hbm_kernel<"


def _pt(w, h, spp, **kw):
    kw.setdefault("num_bounces", 8)
    return m.make_params(w, h, spp, mode=PT, **kw)


@pytest.fixture(scope="module")
def hctx():
    ctx = m.Context(0)
    yield ctx
    ctx.close()


def _pooled_name(ctx, hosek=False, count=False, frame=False, fast=False):
    """The name the launch must report: the geometry is mirt_bvh_pool_plan's for the resident tree."""
    plan = m.bvh_pool_plan(ctx.bvh_info()["plan"]["max_depth"], hosek)
    assert plan["slots"] != 0
    tf = ("false", "true")
    return "%srender_pt_pool_hbm%s_kernel<%d,%d,%d,%s,%s>" % ("fast_build::" if fast else "", "_frame" if frame else "", plan["threads"],
                                                              plan["slots"], 1 if count else 4, tf[count], tf[hosek])


def _strip_and_pooled(ctx, w, h, spp, what, flags=0, **kw):
    """Render without and with MIRT_FLAG_KERNEL_POOL on the context's HBM scene, names asserted; returns the (equal) image."""
    want = ctx.render(_pt(w, h, spp, flags=flags, **kw))
    assert ctx.last_kernel() == STRIP, ctx.last_kernel()
    got = ctx.render(_pt(w, h, spp, flags=flags | POOL, **kw))
    assert ctx.last_kernel() == _pooled_name(ctx), ctx.last_kernel()
    assert_images_equal(got, want, what)
    return got


def _sums(ctx, p):
    ctx.accum_reset(p)
    ctx.accum_add(p)
    return ctx.accum_read(p)


def _field_scene(n, w, h, seed=1, **cam):
    arr, mats, tex = rtiow_field(n, seed=seed)
    cam = cam or dict(eye=(13, 2, 3), at=(0, 0, 0), vfov=30)
    return scene_from_arrays(look(w, h, cam.pop("eye"), cam.pop("at"), **cam), arr, mats, tex), arr


# 1. the schedule is taken with the flag, and only with it
def test_the_flag_selects_the_pooled_kernel(hctx):
    w, h = 64, 40
    hctx.set_scene(scene_data("rtiow_final", w, h), hbm=True)
    for spp in (1, 32, 256):
        hctx.render(_pt(w, h, spp))
        assert hctx.last_kernel() == STRIP, f"default schedule at {spp} spp: {hctx.last_kernel()}"
    hctx.render(_pt(w, h, 32, flags=POOL))
    assert hctx.last_kernel().startswith(POOLED), hctx.last_kernel()
    assert hctx.last_kernel() == _pooled_name(hctx)


# 2. equal to the strip HBM kernel and to the LDS builds
def test_equal_to_strip_and_lds_builds(hctx):
    w, h = 64, 40
    for name, sd in _lds_scenes(w, h):
        hctx.set_scene(sd)
        lds = {spp: hctx.render(_pt(w, h, spp)) for spp in (1, 2, 8, 32)}       # 1: fewer items than a step; 8: slots refill
        lds_sums = _sums(hctx, _pt(w, h, 8))
        hctx.set_scene(sd, hbm=True)
        for spp, want in lds.items():
            assert_images_equal(_strip_and_pooled(hctx, w, h, spp, f"{name} spp{spp}"), want, f"{name} spp{spp} against the LDS build")
        got_sums = _sums(hctx, _pt(w, h, 8, flags=POOL))
        assert hctx.last_kernel() == _pooled_name(hctx)
        assert np.array_equal(got_sums, lds_sums), f"{name}: accumulated sums differ"


def test_frames_bands_and_tiles(hctx):
    sd, _ = _field_scene(3000, 50, 30)
    hctx.set_scene(sd, hbm=True)
    _strip_and_pooled(hctx, 50, 30, 8, "50x30: strips wrap rows, ragged last strips")
    sd, _ = _field_scene(3000, 12, 9)
    hctx.set_scene(sd, hbm=True)
    _strip_and_pooled(hctx, 12, 9, 8, "12x9: narrower than a strip")
    w, h = 64, 48
    sd, _ = _field_scene(3000, w, h)
    hctx.set_scene(sd, hbm=True)
    full = _strip_and_pooled(hctx, w, h, 4, "full frame")
    assert_images_equal(_strip_and_pooled(hctx, w, h, 4, "row band", row_begin=10, row_end=30), full[10:30], "band against the frame")
    part = _strip_and_pooled(hctx, w, h, 4, "tile interleave", tile_rows=4, n_parts=3, part=1)
    p = _pt(w, h, 4, tile_rows=4, n_parts=3, part=1)
    for i in range(part.shape[0]):
        assert np.array_equal(part[i], full[m.params_out_row_index(p, i)]), f"tile row {i}"


# 3. sphere ids beyond 12 and 16 bits
@pytest.mark.parametrize("n", [5000, 70000])
def test_wide_sphere_ids(hctx, oracle, n):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(n)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=25, aperture=0.05), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    got = _strip_and_pooled(hctx, w, h, 4, f"field {n}", num_bounces=6)
    pooled_sums = _sums(hctx, _pt(w, h, 4, num_bounces=6, flags=POOL))
    assert hctx.last_kernel() == _pooled_name(hctx)
    assert np.array_equal(pooled_sums, _sums(hctx, _pt(w, h, 4, num_bounces=6))), f"field {n}: sums against the strip kernel"
    if n == 5000:
        p = _pt(w, h, 4, num_bounces=6)
        assert_images_equal(got, oracle.render(sd, p), "field 5000 against the oracle")
        assert np.array_equal(pooled_sums, oracle.render_pt_sums(sd, p)), "field 5000: sums against the oracle"


# 4. adversarial geometry, against the flat scan
@pytest.mark.parametrize("case", range(5))
def test_adversarial_geometry(hctx, case):
    cases, mats, tex = _adversarial()
    name, arr, eye, at, vfov = cases[case]
    w, h = 48, 32
    hctx.set_scene(scene_from_arrays(look(w, h, eye, at, vfov=vfov), arr, mats, tex), hbm=True)
    got = hctx.render(_pt(w, h, 4, num_bounces=5, flags=POOL))
    assert hctx.last_kernel() == _pooled_name(hctx), hctx.last_kernel()
    flat = hctx.render(_pt(w, h, 4, num_bounces=5, flags=m.MIRT_FLAG_NO_GRID))
    assert hctx.last_kernel().startswith("render_pt_hbm_kernel<false,false,false,"), hctx.last_kernel()
    assert_images_equal(got, flat, f"{name}: pooled BVH against the flat scan")


# 5. counters: a ray's traversal does not depend on the schedule
def test_counters(hctx, oracle):
    w, h = 64, 48
    sd, _ = _field_scene(20000, w, h, seed=4)
    hctx.set_scene(sd, hbm=True)
    count = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID
    want = hctx.render(_pt(w, h, 4, flags=count))
    assert hctx.last_kernel().startswith("render_pt_hbm_kernel<true,false,true,"), hctx.last_kernel()
    ss = hctx.stats()
    got = hctx.render(_pt(w, h, 4, flags=count | POOL))
    assert hctx.last_kernel() == _pooled_name(hctx, count=True), hctx.last_kernel()
    ps = hctx.stats()
    assert_images_equal(got, want, "counting builds")
    for k in ("rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses", "lane_iterations", "grid_cells"):
        assert ps[k] == ss[k], (k, ps[k], ss[k])
    oracle.render(sd, _pt(w, h, 4))
    os_ = oracle.stats()
    for k in ("rays", "hits", "scatter", "sky_misses"):
        assert ps[k] == os_[k], (k, ps[k], os_[k])
    # recorded, not compared: the lane use of the two schedules
    for name, s in (("strip", ss), ("pooled", ps)):
        print(f"\n{name}: traversal lane use {s['grid_cells'] / (64.0 * s['grid_wave_cells']):.3f}, "
              f"step lane use {s['lane_iterations'] / (64.0 * s['wave_iterations']):.3f}")


# 6. bounce limits: 8-bit bounce counters
def test_bounce_limits(hctx):
    w, h = 64, 40
    hctx.set_scene(scene_data("rtiow_final", w, h), hbm=True)
    for nb in (0, 1, 255):
        _strip_and_pooled(hctx, w, h, 4, f"num_bounces {nb}", num_bounces=nb)
    want = hctx.render(_pt(w, h, 4, num_bounces=256))
    got = hctx.render(_pt(w, h, 4, num_bounces=256, flags=POOL))
    assert hctx.last_kernel() == STRIP, hctx.last_kernel()
    assert_images_equal(got, want, "num_bounces 256 is not pooled")


# 7. accumulation and progressive frames
def test_accumulation_and_frames(hctx):
    w, h = 64, 48
    sd, _ = _field_scene(6000, w, h, seed=6)
    hctx.set_scene(sd, hbm=True)
    p24 = _pt(w, h, 24)
    want = hctx.render(p24)
    sums, resolved = [], []
    for flags in (0, POOL):
        p8 = _pt(w, h, 8, flags=flags)
        hctx.accum_reset(p8)
        for _ in range(3):
            hctx.accum_add(p8)
            assert hctx.last_kernel() == (_pooled_name(hctx) if flags else STRIP), hctx.last_kernel()
        assert hctx.accum_samples() == 24
        sums.append(hctx.accum_read(p24))
        resolved.append(hctx.accum_resolve(p24))
    assert np.array_equal(sums[0], sums[1]), "3 x 8 spp: sums"
    assert_images_equal(resolved[1], want, "3 x 8 spp pooled against one 24-spp render")
    assert_images_equal(hctx.render(_pt(w, h, 24, flags=POOL)), want, "24 spp pooled")
    frames, sums = [], []
    for flags in (0, POOL):
        p4 = _pt(w, h, 4, flags=flags)
        hctx.accum_reset(p4)
        imgs = []
        for _ in range(3):
            imgs.append(hctx.accum_frame(p4))
            assert hctx.last_kernel() == (_pooled_name(hctx, frame=True) if flags else "render_pt_hbm_frame_kernel<false,false,true,true>"), hctx.last_kernel()
        sums.append(hctx.accum_read(p4))
        assert_images_equal(hctx.accum_frame(_pt(w, h, 0, flags=flags)), imgs[-1], "a frame with spp == 0 resolves what is there")
        frames.append(imgs)
    assert np.array_equal(sums[0], sums[1]), "frames: sums"
    for k in range(3):
        assert_images_equal(frames[1][k], frames[0][k], f"frame {k}")


# 8. the Hosek sky build; the per-frame RNG stream is not pooled
def test_hosek_sky_and_frame_stream(hctx):
    w, h = 48, 32
    sd = scene_data("rtiow_final", w, h)
    sky = _abi.MirtSkyState()
    for c in range(3):
        for i, v in enumerate([-1.1, -0.3, 0.5, 1.2, -2.5, 0.4, 0.2, 1.5, 0.6]):
            sky.params[9 * c + i] = v * (1.0 + 0.1 * c)
        sky.radiances[c] = 1.0 + c
    sky.sun_direction[:] = [0.0, 0.6, 0.8, 0.0]
    sd.sky = sky
    hctx.set_scene(sd, hbm=True)
    hosek = m.MIRT_FLAG_SKY_HOSEK
    want = hctx.render(_pt(w, h, 8, flags=hosek))
    assert hctx.last_kernel() == "render_pt_hbm_kernel<false,true,true,true>", hctx.last_kernel()
    got = hctx.render(_pt(w, h, 8, flags=hosek | POOL))
    assert hctx.last_kernel() == _pooled_name(hctx, hosek=True), hctx.last_kernel()
    assert_images_equal(got, want, "Hosek sky")
    want = hctx.render(_pt(w, h, 8, frame_spp=2, frame_begin=3))
    got = hctx.render(_pt(w, h, 8, frame_spp=2, frame_begin=3, flags=POOL))
    assert hctx.last_kernel() == STRIP, hctx.last_kernel()
    assert_images_equal(got, want, "frame_spp = 2 is not pooled")


# 9. the stack follows the tree
def test_the_stack_follows_the_tree(hctx):
    w, h = 64, 48
    sd, arr = _field_scene(20000, w, h)
    images = []
    for bvh in ("host", "device"):
        hctx.set_scene(sd, hbm=True, bvh=bvh)
        assert hctx.bvh_info()["built_on_device"] == (bvh == "device")
        images.append(_strip_and_pooled(hctx, w, h, 4, f"{bvh}-built tree"))
    assert_images_equal(images[0], images[1], "host-built against device-built")
    # a shallow tree first, then set_spheres to a deeper one: the stacks are sized by the tree that is resident at the launch
    _, mats, tex = rtiow_field(8)
    copies = sphere_array(np.tile([[0.0, 1.0, 0.0]], (1000, 1)), np.full(1000, 1.0), np.zeros(1000))
    hctx.set_scene(scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), copies, mats, tex), hbm=True)
    shallow = hctx.bvh_info()["plan"]["max_depth"]
    _strip_and_pooled(hctx, w, h, 4, "1 000 copies of one sphere")
    hctx.set_spheres(arr)
    deep = hctx.bvh_info()["plan"]["max_depth"]
    assert deep > shallow, (shallow, deep)
    assert_images_equal(_strip_and_pooled(hctx, w, h, 4, "after set_spheres to a deeper tree"), images[1], "set_spheres against set_scene")
    moved = arr.copy()
    moved["center"][:, 0] = arr["center"][::-1, 0]              # every sphere moves; the topology (and the depth) stays
    moved["center"][:, 1] += 0.25
    hctx.update_spheres(0, moved)
    assert hctx.bvh_info()["plan"]["max_depth"] == deep
    _strip_and_pooled(hctx, w, h, 4, "after update_spheres moved every sphere")


# 10. degenerate trees
def test_degenerate_trees(hctx):
    w, h = 48, 32
    _, mats, tex = rtiow_field(8)
    one = sphere_array([[0.0, 0.0, 0.0]], [1.0], [1])
    hctx.set_scene(scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), one, mats, tex), hbm=True)
    # three spheres whose boxes are not finite: all on the always-tested list, the tree an empty leaf
    cen = np.array([[0.0, -3.0e38, 0.0], [0.0, 1.0, 0.0], [np.nan, 0.0, 0.0]], np.float32)
    rad = np.array([3.0e38, np.inf, 1.0], np.float32)
    assert list(always_list(cen, rad)) == [0, 1, 2]
    worlds = [("no sphere", one[:0], 0), ("one sphere", one, 0), ("three always-tested spheres", sphere_array(cen, rad, [0, 1, 2]), 3)]
    for name, arr, n_always in worlds:
        hctx.set_spheres(arr)
        plan = hctx.bvh_info()["plan"]
        assert plan["n_always"] == n_always and plan["max_depth"] == 0 and plan["n_nodes"] == 0, (name, plan)
        _strip_and_pooled(hctx, w, h, 4, name)


# 11. hints that do not apply
def test_hints_that_do_not_apply(hctx):
    w, h = 64, 40
    hctx.set_scene(scene_data("rtiow_final", w, h), hbm=True)
    want = hctx.render(_pt(w, h, 4))
    flat = hctx.render(_pt(w, h, 4, flags=m.MIRT_FLAG_NO_GRID))
    flat_name = hctx.last_kernel()
    assert flat_name.startswith("render_pt_hbm_kernel<false,false,false,")
    assert_images_equal(hctx.render(_pt(w, h, 4, flags=POOL | m.MIRT_FLAG_NO_GRID)), flat, "POOL | NO_GRID")
    assert hctx.last_kernel() == flat_name
    assert_images_equal(hctx.render(_pt(w, h, 4, flags=POOL | m.MIRT_FLAG_KERNEL_STRIP)), want, "POOL | STRIP")
    assert hctx.last_kernel() == STRIP
    assert_images_equal(hctx.render(_pt(w, h, 4, flags=POOL | m.MIRT_FLAG_TEXEL_TILES)), want, "POOL | TEXEL_TILES")
    assert hctx.last_kernel() == _pooled_name(hctx)
    parity = hctx.render(m.make_params(w, h, 4))
    parity_name = hctx.last_kernel()
    assert parity_name.startswith("render_parity_hbm_kernel<")
    assert_images_equal(hctx.render(m.make_params(w, h, 4, flags=POOL)), parity, "parity mode")
    assert hctx.last_kernel() == parity_name


# 12. fast math: the criterion of test_gpu_fast_math.py::test_fast_math_stays_within_one_unit on its (rtiow_final, 480x270, 64 spp) row,
#     against the exact pooled image
def test_fast_math(hctx):
    w, h, spp = 480, 270, 64
    hctx.set_scene(scene_data("rtiow_final", w, h), hbm=True)
    exact = hctx.render(m.make_params(w, h, spp, mode=PT, flags=POOL))
    assert hctx.last_kernel() == _pooled_name(hctx)
    fast = hctx.render(m.make_params(w, h, spp, mode=PT, flags=POOL | m.MIRT_FLAG_FAST_MATH))
    assert hctx.last_kernel() == _pooled_name(hctx, fast=True), hctx.last_kernel()
    assert hctx.last_kernel().startswith("fast_build::render_pt_pool_hbm_kernel<")
    d = np.abs(exact[..., :3].astype(np.int16) - fast[..., :3].astype(np.int16)).max(axis=-1)
    vals, counts = np.unique(d, return_counts=True)
    hist = {int(v): int(c) for v, c in zip(vals, counts)}
    within1 = (hist.get(0, 0) + hist.get(1, 0)) / (w * h)
    print(f"\nfast-math pooled vs exact pooled: pixels by max |delta| {hist}; within 1: {100.0 * within1:.4f} %")
    assert within1 >= 0.999, hist
    assert (fast[..., 3] == 255).all()
    again = hctx.render(m.make_params(w, h, spp, mode=PT, flags=POOL | m.MIRT_FLAG_FAST_MATH))
    assert_images_equal(again, fast, "the fast-math pooled build is deterministic")
    strip_fast = hctx.render(m.make_params(w, h, spp, mode=PT, flags=m.MIRT_FLAG_FAST_MATH))
    assert hctx.last_kernel() == "fast_build::" + STRIP
    assert_images_equal(fast, strip_fast, "fast-math pooled against fast-math strip")


# 13. a node passes the flag to its members
def test_node(hctx):
    w, h = 64, 48
    sd, _ = _field_scene(8000, w, h, seed=8)
    hctx.set_scene(sd, hbm=True)
    want = _strip_and_pooled(hctx, w, h, 4, "one context")
    node = m.Node([0, 0])
    try:
        node.set_scene(sd, hbm=True)
        assert_images_equal(node.render(_pt(w, h, 4, flags=POOL)), want, "node of 2, pooled")
    finally:
        node.close()
