"""mirt_ctx_set_spheres / _device / mirt_node_set_spheres: a MIRT_SCENE_HBM scene gets a new sphere table -- from host or from device
memory -- and everything set_scene derives from the spheres is derived again on the device.

The contract is one sentence: afterwards the context cannot be told from one that received a fresh set_scene_ex(HBM | BVH_DEVICE) of
the same scene.  `same` holds a context to that: the bytes of the tree, bvh_info, the kernel chosen, images and exact sums."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import bvh_check
from bvh_check import check_bvh
from helpers import assert_images_equal
from hbm_worlds import look, rtiow_field, scene_from_arrays, sphere_array
from set_spheres_worlds import ALWAYS_WORLDS
from test_gpu_bvh_device import _mats, _soup

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
BUILDERS = ("host", "device")
W, H = 16, 16
FIELD_VIEW = dict(eye=(13, 2, 3), at=(0, 0, 0), vfov=25)
COUNT = m.MIRT_FLAG_COUNT_WORK
COUNTERS = ("samples", "rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses", "grid_cells", "grid_wave_cells", "texel_fetches")


def _pt(w=W, h=H, spp=2, **kw):
    kw.setdefault("num_bounces", 8)
    return m.make_params(w, h, spp, mode=PT, **kw)


def _scene(arr, mats=None, **view):
    mt, tex = mats or _mats()
    return scene_from_arrays(look(W, H, view.pop("eye", (0, 0.5, 4)), view.pop("at", (0, 0, -6)), vfov=view.pop("vfov", 50)), arr, mt, tex)


@pytest.fixture(scope="module")
def ctxs():
    """`set`: the context under test;  `fresh`: only ever given whole scenes with HBM | BVH_DEVICE;  `host`: whole scenes, host tree."""
    out = {k: m.Context(0) for k in ("set", "fresh", "host")}
    yield out
    for c in out.values():
        c.close()


def _tree_bytes(ctx):
    return [a.tobytes() for a in ctx.bvh_read()]


def _status(fn):
    try:
        fn()
    except m.MirtError as e:
        return e.status
    return _abi.MIRT_OK


def same(ctx, fresh, what, p=None):
    """`ctx` is indistinguishable from `fresh`: tree bytes, bvh_info, refit count, the kernel, the image and the exact sums."""
    p = p or _pt()
    assert ctx.bvh_info() == fresh.bvh_info(), what
    assert _tree_bytes(ctx) == _tree_bytes(fresh), what
    assert ctx.bvh_refits() == fresh.bvh_refits(), what
    got, want = ctx.render(p), fresh.render(p)
    assert ctx.last_kernel() == fresh.last_kernel() and "hbm" in ctx.last_kernel(), (what, ctx.last_kernel(), fresh.last_kernel())
    assert_images_equal(got, want, f"{what}: set_spheres vs a fresh set_scene_ex(HBM | BVH_DEVICE)")
    sums = []
    for c in (ctx, fresh):
        c.accum_reset(p)
        c.accum_frame(p)
        sums.append(c.accum_read(p))
    assert np.array_equal(sums[0], sums[1]), f"{what}: accumulated sums"
    return got


def _fresh(ctxs, arr, mats=None, **view):
    ctxs["fresh"].set_scene(_scene(arr, mats, **view), hbm=True, bvh="device")
    return ctxs["fresh"]


def _set_over(ctxs, resident, b, arr, what, mats=None, **view):
    """`resident` set with builder b on the context under test, then `arr` by set_spheres; held to a fresh context."""
    ctx = ctxs["set"]
    ctx.set_scene(_scene(resident, mats, **view), hbm=True, bvh=b)
    assert ctx.bvh_info()["built_on_device"] == (1 if b == "device" else 0)
    ctx.set_spheres(arr)
    info = ctx.bvh_info()
    assert info["built_on_device"] == 1 and ctx.bvh_refits() == 0, what
    assert info["plan"]["n_always"] + info["plan"]["n_leaf_spheres"] == len(arr), what
    return ctx


# ---- 1. sizes: leaf roots, the three-sphere copy, the first inner node, wave and block edges; growth and leftovers ----

_ORACLE = {}


@pytest.mark.parametrize("b", BUILDERS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 1025])
def test_sizes(ctxs, oracle, b, n):
    arr = _soup(n, seed=100 + n)
    fresh = _fresh(ctxs, arr)
    ctxs["host"].set_scene(_scene(arr), hbm=True)
    host_img = ctxs["host"].render(_pt())
    if n not in _ORACLE:
        _ORACLE[n] = oracle.render(_scene(arr), _pt())
    for resident in (2 * n + 7, n // 2 if n > 1 else n + 1):        # a larger world (leftovers of its tree), a smaller one (every table grows)
        what = f"n = {n} over {resident} ({b} tree)"
        ctx = _set_over(ctxs, _soup(resident, seed=900 + resident), b, arr, what)
        img = same(ctx, fresh, what)
        assert_images_equal(img, host_img, f"{what}: vs the host tree")
        assert_images_equal(img, _ORACLE[n], f"{what}: vs the oracle")
    nodes, recs, ids = ctx.bvh_read()
    check_bvh(nodes, recs, ids, ctx.bvh_info(), arr["center"][:, :3], arr["radius"])


@pytest.mark.parametrize("b", BUILDERS)
def test_field_of_20000(ctxs, b):
    arr = rtiow_field(20000)[0]
    fresh = _fresh(ctxs, arr, **FIELD_VIEW)
    ctxs["host"].set_scene(_scene(arr, **FIELD_VIEW), hbm=True)
    for resident in (rtiow_field(30000, seed=3)[0], _soup(257, seed=357)):
        what = f"field 20 000 over {len(resident)} ({b} tree)"
        ctx = _set_over(ctxs, resident, b, arr, what, **FIELD_VIEW)
        img = same(ctx, fresh, what)
        assert_images_equal(img, ctxs["host"].render(_pt()), f"{what}: vs the host tree")
    nodes, recs, ids = ctx.bvh_read()
    count = check_bvh(nodes, recs, ids, ctx.bvh_info(), arr["center"][:, :3], arr["radius"])
    assert count["n_always"] == 5 and count["n_nodes"] > 4 * 256


def test_field_of_100000_against_the_flat_scan(ctxs):
    arr = rtiow_field(100000)[0]
    ctx = _set_over(ctxs, rtiow_field(5000)[0], "device", arr, "field 100 000", **FIELD_VIEW)
    got = ctx.render(_pt())
    assert_images_equal(got, ctx.render(_pt(flags=m.MIRT_FLAG_NO_GRID)), "field 100 000: the tree vs the flat scan of the table in device memory")
    same(ctx, _fresh(ctxs, arr, **FIELD_VIEW), "field 100 000")


# ---- 2. one context, world after world ----

def test_the_chain(ctxs, oracle):
    ctx = ctxs["set"]
    ctx.set_scene(_scene(_soup(100, seed=200)), hbm=True)
    for n in (1025, 5, 0, 65):
        arr = _soup(n, seed=300 + n)
        ctx.set_spheres(arr)
        img = same(ctx, _fresh(ctxs, arr), f"chain: {n}")
        if n == 0:
            sky = oracle.render(_scene(arr), _pt())
            assert_images_equal(img, sky, "the empty world renders the sky")
            assert ctx.bvh_info()["plan"]["device_bytes"] == 0


# ---- 3. the always-tested list where the rule has edges ----

@pytest.mark.parametrize("b", BUILDERS)
@pytest.mark.parametrize("name", list(ALWAYS_WORLDS))
def test_the_always_list(ctxs, b, name):
    build, claimed = ALWAYS_WORLDS[name]
    arr = build()
    ctx = _set_over(ctxs, _soup(65, seed=165), b, arr, name)
    info = ctx.bvh_info()
    ids = ctx.bvh_read()[2]
    want = bvh_check.always_list(arr["center"][:, :3], arr["radius"])
    assert info["plan"]["n_always"] == claimed == len(want), name
    assert np.array_equal(ids[:claimed].astype(np.int64), want), name
    same(ctx, _fresh(ctxs, arr), name)


# ---- 4. what the materials decide ----

def _using(n, choices, seed):
    arr = _soup(n, seed=seed)
    arr["material_idx"] = np.asarray(choices, np.uint32)[np.random.default_rng(seed).integers(0, len(choices), n)]
    return arr


def test_the_routines_in_use_follow_the_spheres(ctxs):
    ctx = ctxs["set"]
    ctx.set_scene(_scene(_soup(65, seed=165)), hbm=True, bvh="device")
    worlds = [("lambertian only", _using(257, [0, 5], 41)), ("every routine and id 7", _using(300, range(7), 42)), ("lambertian again", _using(65, [5], 43)),
              ("an image texture", _using(65, [1], 44)), ("metal and glass", _using(3, [2, 3], 45))]
    for what, arr in worlds:
        ctx.set_spheres(arr)
        fresh = _fresh(ctxs, arr)
        same(ctx, fresh, what)
        for flags in (COUNT, COUNT | m.MIRT_FLAG_COUNT_GRID, m.MIRT_FLAG_TEXEL_TILES, m.MIRT_FLAG_KERNEL_POOL):
            p = _pt(spp=16, flags=flags)
            assert_images_equal(ctx.render(p), fresh.render(p), f"{what}: flags {flags:#x}")
            assert ctx.last_kernel() == fresh.last_kernel(), what
            if flags & COUNT:
                got, want = ctx.stats(), fresh.stats()
                assert [got[k] for k in COUNTERS] == [want[k] for k in COUNTERS], f"{what}: counters, flags {flags:#x}"


def test_a_material_index_out_of_range_is_the_render_calls_error(ctxs):
    ctx = ctxs["set"]
    good = _soup(65, seed=165)
    ctx.set_scene(_scene(good), hbm=True)
    bad = _soup(257, seed=357)
    bad["material_idx"][200] = len(_mats()[0])
    assert m.lib().mirt_ctx_set_spheres(ctx._h, bad.ctypes.data_as(C.c_void_p), len(bad)) == _abi.MIRT_OK
    fresh = _fresh(ctxs, bad)
    for c in (ctx, fresh):
        assert _status(lambda: c.render(_pt())) == _abi.MIRT_ERR_MATERIAL_INDEX
        assert _status(lambda: c.accum_frame(_pt())) == _abi.MIRT_ERR_MATERIAL_INDEX
    assert ctx.bvh_info() == fresh.bvh_info() and _tree_bytes(ctx) == _tree_bytes(fresh)
    parity = m.make_params(W, H, 2, mode=m.MIRT_MODE_PARITY)
    assert_images_equal(ctx.render(parity), fresh.render(parity), "parity mode does not read the spheres' materials")
    ctx.set_spheres(good)
    same(ctx, _fresh(ctxs, good), "a good world after one with a bad index")


def test_the_materials_own_verdict_stays(ctxs):
    mats, tex = _mats()
    broken = [_abi.MirtMaterial.from_buffer_copy(bytes(x)) for x in mats]
    broken[5].desc1.offset = len(tex) + 3                          # a lambertian's texel beyond the table
    table = (broken, tex)
    ctx = ctxs["set"]
    a, b = _soup(65, seed=165), _using(257, [0, 2], 46)            # b does not even use material 5
    ctx.set_scene(_scene(a, table), hbm=True)
    assert _status(lambda: ctx.render(_pt())) == _abi.MIRT_ERR_TEXEL_RANGE
    ctx.set_spheres(b)
    fresh = _fresh(ctxs, b, table)
    for c in (ctx, fresh):
        assert _status(lambda: c.render(_pt())) == _abi.MIRT_ERR_TEXEL_RANGE
    b["material_idx"][7] = 99                                      # the spheres are checked first
    ctx.set_spheres(b)
    fresh = _fresh(ctxs, b, table)
    for c in (ctx, fresh):
        assert _status(lambda: c.render(_pt())) == _abi.MIRT_ERR_MATERIAL_INDEX
    ctx.set_spheres(a)
    assert _status(lambda: ctx.render(_pt())) == _abi.MIRT_ERR_TEXEL_RANGE
    # parity mode reads material 2 on every hit of a world that is not empty
    two = (list(mats[:2]), tex)
    ctx.set_scene(_scene(a[:0], two), hbm=True)
    parity = m.make_params(W, H, 2, mode=m.MIRT_MODE_PARITY)
    sky = ctx.render(parity)
    a0 = a.copy()
    a0["material_idx"] %= 2
    ctx.set_spheres(a0)
    fresh = _fresh(ctxs, a0, two)
    for c in (ctx, fresh):
        assert _status(lambda: c.render(parity)) == _abi.MIRT_ERR_MATERIAL_INDEX
    ctx.set_spheres(a0[:0])
    assert_images_equal(ctx.render(parity), sky, "parity mode of the empty world again")


# ---- 5. the device-pointer variant ----

@pytest.mark.parametrize("b", BUILDERS)
def test_device_pointer(ctxs, oracle, b):
    import torch
    arr = ALWAYS_WORLDS["80 big"][0]()
    arr = np.concatenate([arr, _soup(257, seed=357)])
    ctx = _set_over(ctxs, _soup(65, seed=165), b, arr, "host pointer")
    want, want_img = _tree_bytes(ctx), ctx.render(_pt())
    garbage = arr.copy()
    garbage["_pad"] = 0xffffffff
    garbage["center"][:, 3] = np.nan
    buf = np.zeros(32 * len(arr) + 16, np.uint8)
    buf[4:4 + 32 * len(arr)] = garbage.view(np.uint8)
    d = torch.from_numpy(buf).to("cuda:0")
    ptr = d.data_ptr() + 4
    assert ptr % 16 == 4
    ctx.set_scene(_scene(_soup(65, seed=165)), hbm=True, bvh=b)
    for call in range(2):
        ctx.set_spheres_device(len(arr), ptr)
        assert _tree_bytes(ctx) == want, f"device pointer, call {call}"
        assert_images_equal(ctx.render(_pt()), want_img, "device pointer vs host pointer")
    same(ctx, _fresh(ctxs, arr), "device pointer")
    assert_images_equal(want_img, oracle.render(_scene(arr), _pt()), "device pointer vs the oracle")
    assert torch.equal(d.cpu(), torch.from_numpy(buf)), "the source is only read"
    ctx.set_spheres_device(0, 0)                                    # the empty world needs no pointer
    same(ctx, _fresh(ctxs, arr[:0]), "device pointer, empty")


# ---- 6. after it, everything else ----

def test_the_other_calls_after_a_set_spheres(ctxs, oracle):
    w, h = 32, 24
    arr = _soup(257, seed=357)
    arr["radius"][[100, 130]] = 3.0
    ctx = _set_over(ctxs, _soup(1025, seed=1125), "host", arr, "before the other calls")
    fresh = _fresh(ctxs, arr)
    moved = arr.copy()
    moved["center"][90:140, :3] += np.float32(0.2)
    moved["radius"][90:140] *= np.float32(1.1)
    for c in (ctx, fresh):
        assert c.bvh_refits() == 0
        c.update_spheres(90, moved[90:140])
        assert c.bvh_refits() == 1
    img = same(ctx, fresh, "update_spheres after set_spheres")
    ctxs["host"].set_scene(_scene(moved), hbm=True)
    assert_images_equal(img, ctxs["host"].render(_pt()), "update_spheres after set_spheres vs a fresh host tree of the moved world")
    ctx.set_spheres(arr)
    fresh = _fresh(ctxs, arr)
    assert ctx.bvh_refits() == 0
    parity = m.make_params(w, h, 2, mode=m.MIRT_MODE_PARITY)
    got = ctx.render(parity)
    assert ctx.last_kernel().startswith("render_parity_hbm_kernel"), ctx.last_kernel()
    assert_images_equal(got, fresh.render(parity), "parity mode")
    assert_images_equal(got, oracle.render(_scene(arr), parity), "parity mode vs the oracle")
    out = {}
    for name, c in (("set", ctx), ("fresh", fresh)):
        p = _pt(w, h, 2)
        c.accum_reset(p)
        frames = [c.accum_frame(p), c.accum_frame(p)]
        kernels = [c.last_kernel()]
        sums = c.accum_read(p)
        pf = _pt(w, h, 2, seed=4, frame_spp=2, frame_begin=7)       # the reference's stream: one RNG stream per pixel and frame
        c.accum_reset(pf)
        frames += [c.accum_frame(pf), c.accum_frame(pf)]
        sums = np.concatenate([sums.ravel(), c.accum_read(pf).ravel()])
        imgs = [c.render(_pt(w, h, 4, frame_spp=2, frame_begin=3)), c.render(_pt(w, h, 2, flags=m.MIRT_FLAG_FAST_MATH))]
        kernels.append(c.last_kernel())
        stats = []
        for flags in (COUNT, COUNT | m.MIRT_FLAG_COUNT_GRID):
            imgs.append(c.render(_pt(w, h, 2, flags=flags)))
            kernels.append(c.last_kernel())
            st = c.stats()
            stats.append([st[k] for k in COUNTERS])
        out[name] = (frames + imgs, sums, kernels, stats)
    assert "render_pt_hbm_frame_kernel" in out["set"][2][0] and out["set"][2][1].startswith("fast_build::"), out["set"][2]
    for i, (a, b) in enumerate(zip(out["set"][0], out["fresh"][0])):
        assert_images_equal(a, b, f"image {i} of: two frames, two frames with frame_spp = 2, a launch with frame_spp = 2, fast math, counted flat scan, counted tree")
    assert np.array_equal(out["set"][1], out["fresh"][1]), "sums"
    assert out["set"][2] == out["fresh"][2] and out["set"][3] == out["fresh"][3]
    assert out["set"][3][0][2] > out["set"][3][1][2] > 0            # the tree tests fewer spheres than the flat scan


# ---- 7. refusals change nothing ----

def test_refusals_change_nothing(ctxs):
    lib = m.lib()
    a = _soup(65, seed=165)
    ptr = a.ctypes.data_as(C.c_void_p)
    nowhere = C.c_void_p(0x10)                                      # must not be read
    calls = (lib.mirt_ctx_set_spheres, lib.mirt_ctx_set_spheres_device)
    with m.Context(0) as empty:                                     # before any scene
        for fn in calls:
            assert fn(empty._h, ptr, 1) == _abi.MIRT_ERR_NO_SCENE
            assert fn(empty._h, None, 0) == _abi.MIRT_ERR_NO_SCENE
    ctx = ctxs["set"]
    ctx.set_scene(_scene(a))                                        # an LDS scene
    want = ctx.render(_pt())
    for fn in calls:
        assert fn(ctx._h, ptr, len(a)) == _abi.MIRT_ERR_NO_SCENE
    assert _status(lambda: ctx.set_spheres(a)) == _abi.MIRT_ERR_NO_SCENE
    assert_images_equal(ctx.render(_pt()), want, "an LDS scene after a refused set_spheres")
    for b in BUILDERS:
        ctx.set_scene(_scene(a), hbm=True, bvh=b)
        ctx.update_spheres(0, a[:2])
        want, tree, info = ctx.render(_pt()), _tree_bytes(ctx), ctx.bvh_info()
        for p, n, status in ((None, 1, _abi.MIRT_ERR_NULL_POINTER), (None, len(a), _abi.MIRT_ERR_NULL_POINTER),
                             (nowhere, 2 ** 24 + 1, _abi.MIRT_ERR_SCENE_TOO_LARGE), (nowhere, 2 ** 32 - 1, _abi.MIRT_ERR_SCENE_TOO_LARGE)):
            for fn in calls:
                assert fn(ctx._h, p, n) == status, (n, status)
            assert _tree_bytes(ctx) == tree and ctx.bvh_info() == info and ctx.bvh_refits() == 1
            assert_images_equal(ctx.render(_pt()), want, f"after the refused set_spheres of {n}")
        ctx.update_spheres(0, a[:2])                                # the refit's tables survived the refusals
        assert ctx.bvh_refits() == 2 and _tree_bytes(ctx) == tree


# ---- 8. node ----

@pytest.mark.parametrize("members", [2, 4])
def test_node_loopback(ctxs, members):
    w, h = 32, 24
    a, bb = _soup(257, seed=357), _soup(1025, seed=1125)
    ctxs["fresh"].set_scene(_scene(bb), hbm=True, bvh="device")
    want = ctxs["fresh"].render(_pt(w, h))
    tree = _tree_bytes(ctxs["fresh"])
    with m.Node([0] * members) as node:
        lib, ptr = m.lib(), bb.ctypes.data_as(C.c_void_p)
        assert lib.mirt_node_set_spheres(node._h, ptr, 1) == _abi.MIRT_ERR_NO_SCENE
        node.set_scene(_scene(a), hbm=True, bvh="host" if members == 2 else "device")
        assert lib.mirt_node_set_spheres(node._h, None, 1) == _abi.MIRT_ERR_NULL_POINTER
        assert lib.mirt_node_set_spheres(node._h, C.c_void_p(0x10), 2 ** 24 + 1) == _abi.MIRT_ERR_SCENE_TOO_LARGE
        node.set_spheres(bb)
        assert_images_equal(node.render(_pt(w, h)), want, f"node of {members} after set_spheres")
        for i in range(members):
            assert node.context(i).bvh_info()["built_on_device"] == 1 and _tree_bytes(node.context(i)) == tree
        node.set_spheres(bb[:0])
        assert node.context(members - 1).bvh_info()["plan"]["device_bytes"] == 0
        node.set_scene(_scene(a))                                   # an LDS scene on every member
        assert lib.mirt_node_set_spheres(node._h, ptr, 1) == _abi.MIRT_ERR_NO_SCENE
        assert node.render(_pt(w, h)).shape == want.shape           # a refused call leaves the node its scene


# ---- 9. the host objects ----

def _objects(n, seed):
    arr = rtiow_field(n, seed=seed)[0]
    return [m.Sphere(arr["center"][i, :3], float(arr["radius"][i]), int(arr["material_idx"][i]) % 3) for i in range(n)]


_OBJECT_MATS = lambda: [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))), m.Material.Metal(albedo=m.Texture.new_from_color((0.7, 0.6, 0.5)), fuzz=0.2),
                        m.Material.Lambertian(albedo=m.Texture.new_from_color((0.8, 0.3, 0.2)))]         # parity mode reads material 2's texture on every hit
_OBJECT_CAM = lambda: m.Camera(np.asarray((13, 2, 3), np.float32), np.asarray((-0.96, -0.1, -0.22), np.float32), np.asarray((0, 1, 0), np.float32),
                               m.Angle.degrees(25.0), 0.0, 10.0)


def test_raytracer_set_world():
    """A world beyond the LDS budget is in device memory: set_world replaces its spheres in place and restarts the accumulation; a
    small world is set again.  Either way the frames are those of a Raytracer made from the new scene."""
    rp = m.RenderParams(camera=_OBJECT_CAM(), sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=2, num_bounces=4), viewport_size=(32, 24))
    for n, k, in_place in ((5000, 4300, True), (40, 30, False)):
        old, new = _objects(n, 1), _objects(k, 2)
        rt = m.Raytracer(m.Scene(old, _OBJECT_MATS()), rp)
        try:
            rt.render_frame()
            rt.set_world(new)
            assert rt.progress() == 0.0 and len(rt.spheres) == k and rt._hbm is in_place
            if in_place:
                assert rt._ctx.bvh_info()["built_on_device"] == 1 and rt._ctx.bvh_refits() == 0
            got = [rt.render_frame(), rt.render_frame()]
        finally:
            rt.close()
        rt = m.Raytracer(m.Scene(new, _OBJECT_MATS()), rp)
        try:
            rt.render_frame()                                        # the frames of the other are numbered from 2 (reference_stream off: no effect)
            rt.set_render_params(rp)
            for i in range(2):
                assert_images_equal(got[i], rt.render_frame(), f"n = {n} -> {k}: frame {i} after set_world")
        finally:
            rt.close()


def test_layer_set_world():
    rp = m.RenderParams(camera=_OBJECT_CAM(), viewport_size=(32, 24))
    old, new = _objects(5000, 1), _objects(4300, 2)
    layer = m.Layer.new([32, 24], rp, scene=m.Scene(old, _OBJECT_MATS()))
    other = m.Layer.new([32, 24], rp, scene=m.Scene(new, _OBJECT_MATS()))
    try:
        for la in (layer, other):
            la.set_global_data()
            la.set_data(rp)
        assert layer._hbm and not np.array_equal(layer.register_texture(), other.register_texture())
        layer.set_world(new, rp)
        assert layer._ctx.bvh_info()["built_on_device"] == 1 and len(layer.world) == 4300
        assert_images_equal(layer.register_texture(), other.register_texture(), "Layer.set_world vs a Layer of the new world")
    finally:
        layer.close()
        other.close()


@pytest.mark.parametrize("n, k, on_device", [(5000, 4300, 1), (40, 30, 0)])
def test_cpp_set_world(n, k, on_device):
    """The C++ mirror's Raytracer::set_world, Layer::set_world and mirt_host::set_spheres (host/set_world_demo.cpp compares each with an
    object made from the new scene): in place for a world in device memory, by set_scene for a small one."""
    host = Path(__file__).resolve().parent.parent / "weekend-raytracer-wgpu_amd" / "host"
    subprocess.run(["make", "-C", str(host)], check=True, capture_output=True)
    r = subprocess.run([str(host / "set_world_demo"), str(n), str(k), "48", "32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.strip().splitlines()
    tail = f"equal built_on_device {on_device} spheres {k if on_device else 0}"
    assert lines[:2] == [f"raytracer: {tail}", f"layer: {tail}"], r.stdout
    assert lines[2:] == ([f"set_spheres: equal built_on_device 1 spheres {n}"] if on_device else []), r.stdout
