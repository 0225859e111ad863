"""mirt_ctx_update_spheres / _device / mirt_node_update_spheres: the spheres of a MIRT_SCENE_HBM scene moved in place, the BVH refitted on
the device.

The topology, the ids table and the always-tested list stay what they were when the scene was set; what must hold after an update is
what the exactness argument of DESIGN.md 10.1 needs: records are {centre, r * r}, every child box EQUALS the union below it
(tests/bvh_check.py with the always list of the scene as it was set), the bounds bound, and the image is byte for byte the image of a
context that was given the moved world afresh (host tree), of the flat scan, and -- up to 1 025 spheres -- of the oracle."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import bvh_check
from bvh_check import check_bvh
from helpers import assert_images_equal, scene_data
from hbm_worlds import look, rtiow_field, scene_from_arrays, sphere_array
from test_gpu_bvh_device import _mats, _soup

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
BUILDERS = ("host", "device")
W, H = 16, 16
CLAMP = float(np.float32(3.0e38))


def _pt(w=W, h=H, spp=2, **kw):
    kw.setdefault("num_bounces", 8)
    return m.make_params(w, h, spp, mode=PT, **kw)


def _scene(arr, w=W, h=H, eye=(0, 0.5, 4), at=(0, 0, -6), vfov=50):
    mats, tex = _mats()
    return scene_from_arrays(look(w, h, eye, at, vfov=vfov), arr, mats, tex)


FIELD_VIEW = dict(eye=(13, 2, 3), at=(0, 0, 0), vfov=25)


@pytest.fixture(scope="module")
def ctxs():
    """One context per builder, and `fresh`: the context that is only ever given whole worlds (host tree) -- the reference image."""
    out = {b: m.Context(0) for b in BUILDERS + ("fresh",)}
    yield out
    for c in out.values():
        c.close()


def _jitter(arr, seed, amount=0.3):
    rng = np.random.default_rng(seed)
    out = arr.copy()
    out["center"][:, :3] += rng.uniform(-amount, amount, (len(arr), 3)).astype(np.float32)
    out["radius"] *= rng.uniform(0.8, 1.2, len(arr)).astype(np.float32)
    return out


def _tree_bytes(ctx):
    return [a.tobytes() for a in ctx.bvh_read()]


class Moved:
    """A world set on `ctx` with builder `b`, then updated step by step; every step runs the checks of `check_moved`."""

    def __init__(self, ctxs, b, world, monkeypatch, oracle=None, w=W, h=H, view=None, params=None):
        self.ctx, self.fresh, self.b, self.oracle, self.mp = ctxs[b], ctxs["fresh"], b, oracle, monkeypatch
        self.w, self.h, self.view = w, h, view or {}
        self.p = params or _pt(w, h)
        self.now = world.copy()
        self.ctx.set_scene(self.scene(world), hbm=True, bvh=b)
        info = self.ctx.bvh_info()
        assert info["built_on_device"] == (1 if b == "device" else 0)
        self.plan = info["plan"]
        self.first_read = _tree_bytes(self.ctx)
        self.first_info = info
        self.always = self.ctx.bvh_read()[2][:self.plan["n_always"]].astype(np.int64)
        self.refits = 0
        assert self.ctx.bvh_refits() == 0

    def scene(self, arr):
        return _scene(arr, self.w, self.h, **self.view)

    def host_update(self, first, recs):
        self.ctx.update_spheres(first, recs)

    def step(self, first, recs, what, update=None, structure=True, oracle=True, fresh=True):
        """Spheres first .. take centre and radius from `recs`; then the checks."""
        (update or self.host_update)(first, recs)
        self.refits += 1
        self.now["center"][first:first + len(recs)] = recs["center"]
        self.now["radius"][first:first + len(recs)] = recs["radius"]
        self.check(what, structure, oracle, fresh)

    def check(self, what, structure=True, oracle=True, fresh=True):
        ctx, now = self.ctx, self.now
        what = f"{what} ({self.b} tree, n = {len(now)})"
        info = ctx.bvh_info()
        assert ctx.bvh_refits() == self.refits, what
        assert info["plan"] == self.plan and info["root"] == self.first_info["root"], what
        if structure:
            nodes, recs, ids = ctx.bvh_read()
            self.mp.setattr(bvh_check, "always_list", lambda centres, radii: self.always)
            check_bvh(nodes, recs, ids, info, now["center"][:, :3], now["radius"])
            self.mp.undo()
        got = ctx.render(self.p)
        assert "hbm" in ctx.last_kernel(), ctx.last_kernel()
        flat = m.make_params(self.w, self.h, self.p.spp, mode=PT, num_bounces=self.p.num_bounces, flags=m.MIRT_FLAG_NO_GRID)
        assert_images_equal(got, ctx.render(flat), f"{what}: refitted tree vs the same context's flat scan")
        if fresh:
            self.fresh.set_scene(self.scene(now), hbm=True)
            assert_images_equal(got, self.fresh.render(self.p), f"{what}: refitted tree vs a fresh host tree of the moved world")
        if oracle and self.oracle is not None and len(now) <= 1025:
            assert_images_equal(got, self.oracle.render(self.scene(now), self.p), f"{what}: refitted tree vs oracle")
        return got


# ---- sizes: a leaf root, the three-sphere copy, the first inner node, wave and block edges ----

@pytest.mark.parametrize("b", BUILDERS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 65, 257, 1025])
def test_every_sphere_jittered(ctxs, oracle, monkeypatch, b, n):
    a = _soup(n, seed=100 + n)
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    mv.step(0, _jitter(a, 200 + n), "all centres and radii jittered")
    assert bool(mv.first_info["root"] & m.BVH_LEAF) == (n <= 4)


@pytest.mark.parametrize("b", BUILDERS)
def test_field_of_20000(ctxs, monkeypatch, b):
    """Levels of several blocks, a deep tree.  (check_bvh walks its ~7 000 nodes in about a second.)"""
    a = rtiow_field(20000)[0]
    mv = Moved(ctxs, b, a, monkeypatch, w=64, h=48, view=FIELD_VIEW)
    bb = _jitter(a, 7, amount=0.1)
    bb[:5] = a[:5]
    mv.step(0, bb, "field 20 000")
    assert mv.plan["n_nodes"] > 4 * 256


# ---- partial ranges ----

def _soup_with_big(n=257):
    a = _soup(n, seed=100 + n)
    a["radius"][[100, 130]] = 3.0                                  # above 4 median radii: always tested
    return a


@pytest.mark.parametrize("b", BUILDERS)
def test_partial_ranges(ctxs, oracle, monkeypatch, b):
    a = _soup_with_big()
    bb = _jitter(a, 1)
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    assert mv.always.tolist() == [100, 130]
    for first, count in ((0, 1), (256, 1), (90, 50)):               # the last one crosses both always-tested spheres
        mv.step(first, bb[first:first + count], f"range ({first}, {count})")
    # count == 0 is a no-op, wherever it points and whatever it is given
    before = _tree_bytes(mv.ctx)
    lib = m.lib()
    for first, ptr in ((0, None), (257, None), (5, bb.ctypes.data_as(C.c_void_p))):
        assert lib.mirt_ctx_update_spheres(mv.ctx._h, first, 0, ptr) == 0
        assert lib.mirt_ctx_update_spheres_device(mv.ctx._h, first, 0, ptr) == 0
    mv.ctx.update_spheres(3, bb[:0])
    assert _tree_bytes(mv.ctx) == before and mv.ctx.bvh_refits() == mv.refits


# ---- worlds that make a refitted tree bad, never wrong ----

@pytest.mark.parametrize("b", BUILDERS)
def test_teleport(ctxs, oracle, monkeypatch, b):
    """Every centre goes to another sphere's place: every box overlaps every other.  Bytes only."""
    a = _soup(257, seed=357)
    bb = a.copy()
    bb["center"] = a["center"][np.random.default_rng(3).permutation(len(a))]
    Moved(ctxs, b, a, monkeypatch, oracle).step(0, bb, "teleport")


@pytest.mark.parametrize("b", BUILDERS)
def test_always_listed_spheres_move_and_a_tree_sphere_grows(ctxs, oracle, monkeypatch, b):
    a = rtiow_field(1000)[0]
    mv = Moved(ctxs, b, a, monkeypatch, oracle, w=32, h=24, view=FIELD_VIEW)
    assert mv.always.tolist() == [0, 1, 2, 3, 4]
    bb = a[:12].copy()
    bb["center"][0, 1] -= 0.5                                       # the ground sinks,
    bb["center"][1:5, 0] += 1.25                                    # the heroes move,
    bb["radius"][1] = 1.5
    bb["radius"][10] = 50.0                                         # and a tree sphere becomes far larger than them: it stays in the tree
    r_max_before = mv.first_info["r_max"]
    mv.step(0, bb, "ground, heroes and a grown tree sphere")
    info = mv.ctx.bvh_info()
    assert r_max_before < 1.0 and 50.0 <= info["r_max"] <= 50.001
    assert info["radius"] > mv.first_info["radius"]
    assert mv.ctx.bvh_read()[2][:5].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("b", BUILDERS)
def test_negative_and_zero_radius(ctxs, oracle, monkeypatch, b):
    a = _soup(65, seed=165)
    bb = a[5:12].copy()
    bb["radius"][2] = -0.3
    bb["radius"][4] = 0.0
    Moved(ctxs, b, a, monkeypatch, oracle).step(5, bb, "a negative and a zero radius in the tree")


@pytest.mark.parametrize("b", BUILDERS)
def test_non_finite_and_back(ctxs, oracle, monkeypatch, b):
    a = _soup(65, seed=165)
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    assert len(mv.always) == 0
    bb = a[20:23].copy()
    bb["center"][0, 1] = np.nan
    bb["center"][1, 0] = np.inf
    bb["radius"][2] = np.inf
    mv.step(20, bb, "NaN centre, inf centre, inf radius", oracle=False)
    nodes = mv.ctx.bvh_read()[0]
    assert mv.ctx.bvh_info()["radius"] == CLAMP
    assert np.isinf(nodes["lmin"]).any() or np.isinf(nodes["rmin"]).any()
    assert np.isinf(nodes["lmax"]).any() or np.isinf(nodes["rmax"]).any()
    mv.step(20, _jitter(a, 9)[20:23], "finite again")
    info = mv.ctx.bvh_info()
    assert np.isfinite(info["radius"]) and info["radius"] < 100.0
    assert np.isfinite(mv.ctx.bvh_read()[0]["lmin"]).all()


# ---- determinism ----

@pytest.mark.parametrize("b", BUILDERS)
def test_round_trip(ctxs, oracle, monkeypatch, b):
    a = _soup_with_big()
    bb = _jitter(a, 4)
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    mv.step(0, bb, "A -> B")
    at_b, info_b = _tree_bytes(mv.ctx), mv.ctx.bvh_info()
    mv.step(0, bb, "B again", oracle=False)
    assert _tree_bytes(mv.ctx) == at_b and mv.ctx.bvh_info() == info_b
    mv.step(0, a, "B -> A")
    assert _tree_bytes(mv.ctx) == mv.first_read
    if b == "device":
        assert mv.ctx.bvh_info() == mv.first_info                  # (a host tree's own bounds may differ from the reductions': check_bvh's conditions hold)
    mv.step(0, bb, "A -> B again", oracle=False, fresh=False)
    assert _tree_bytes(mv.ctx) == at_b and mv.ctx.bvh_info() == info_b


# ---- the device-pointer variant, and what the input's other words do ----

@pytest.mark.parametrize("b", BUILDERS)
def test_device_pointer(ctxs, oracle, monkeypatch, b):
    import torch
    a = _soup_with_big()
    bb = _jitter(a, 5)
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    mv.step(0, bb, "host pointer")
    want, want_img = _tree_bytes(mv.ctx), mv.ctx.render(mv.p)
    garbage = bb.copy()
    garbage["material_idx"] = 0xdeadbeef
    garbage["_pad"] = 0x7fc00000
    garbage["center"][:, 3] = np.nan
    d = torch.from_numpy(garbage.view(np.uint8).copy()).to("cuda:0")
    assert d.numel() == 32 * len(bb)

    def from_device(first, recs):
        mv.ctx.update_spheres_device(first, len(recs), d.data_ptr() + 32 * first)

    mv2 = Moved(ctxs, b, a, monkeypatch, oracle)
    mv2.step(0, bb, "device pointer, all", update=from_device)
    assert _tree_bytes(mv2.ctx) == want
    assert_images_equal(mv2.ctx.render(mv2.p), want_img, "device pointer vs host pointer")
    mv3 = Moved(ctxs, b, a, monkeypatch, oracle)
    mv3.step(90, bb[90:140], "device pointer, a range", update=from_device, oracle=False)
    mv3.step(0, bb[:90], "device pointer, the head", update=from_device, oracle=False, fresh=False)
    mv3.step(140, bb[140:], "device pointer, the tail", update=from_device, oracle=False, fresh=False)
    assert _tree_bytes(mv3.ctx) == want


@pytest.mark.parametrize("b", BUILDERS)
def test_material_idx_of_the_input_is_not_read(ctxs, oracle, monkeypatch, b):
    a = _soup(65, seed=165)
    bb = _jitter(a, 6)
    other = bb.copy()
    other["material_idx"] = (bb["material_idx"] + 3) % 7
    other["_pad"] = 0xffffffff
    mv = Moved(ctxs, b, a, monkeypatch, oracle)
    mv.step(0, other, "another material_idx in the input")          # mv.now keeps A's materials: fresh tree and oracle render those
    assert np.array_equal(mv.now["material_idx"], a["material_idx"])


# ---- the other kernels of an HBM scene after an update ----

@pytest.mark.parametrize("b", BUILDERS)
def test_parity_accum_frames_and_fast_math_after_an_update(ctxs, oracle, monkeypatch, b):
    w, h = 32, 24
    a = _soup(257, seed=357)
    mv = Moved(ctxs, b, a, monkeypatch, oracle, w=w, h=h)
    mv.step(0, _jitter(a, 8), "before the other kernels")
    ctx, fresh = mv.ctx, mv.fresh                                   # `fresh` holds the moved world since that step
    sd = mv.scene(mv.now)
    parity = m.make_params(w, h, 2, mode=m.MIRT_MODE_PARITY)
    got = ctx.render(parity)
    assert ctx.last_kernel().startswith("render_parity_hbm_kernel"), ctx.last_kernel()
    assert_images_equal(got, oracle.render(sd, parity), "parity mode after an update vs oracle")
    out = {}
    for name, c in (("updated", ctx), ("fresh", fresh)):
        p = _pt(w, h, 2)
        c.accum_reset(p)
        frames = [c.accum_frame(p), c.accum_frame(p)]
        if name == "updated":
            assert "render_pt_hbm_frame_kernel" in c.last_kernel(), c.last_kernel()
        out[name] = (frames, c.accum_read(p), c.render(_pt(w, h, 4, frame_spp=2, frame_begin=3)),
                     c.render(_pt(w, h, 2, flags=m.MIRT_FLAG_FAST_MATH)))
        if name == "updated":
            assert c.last_kernel().startswith("fast_build::"), c.last_kernel()
    for i in range(2):
        assert_images_equal(out["updated"][0][i], out["fresh"][0][i], f"accum_frame {i} after an update")
    assert np.array_equal(out["updated"][1], out["fresh"][1]), "sums after an update"
    assert_images_equal(out["updated"][2], out["fresh"][2], "frame_spp = 2 after an update")
    assert_images_equal(out["updated"][3], out["fresh"][3], "MIRT_FLAG_FAST_MATH after an update")


# ---- errors ----

def test_errors_change_nothing(ctxs):
    lib = m.lib()
    ctx = ctxs["device"]
    a = _soup(65, seed=165)
    n = len(a)
    ptr = a.ctypes.data_as(C.c_void_p)
    with m.Context(0) as empty:                                     # before any scene
        assert lib.mirt_ctx_update_spheres(empty._h, 0, 1, ptr) == _abi.MIRT_ERR_NO_SCENE
        assert lib.mirt_ctx_update_spheres_device(empty._h, 0, 1, ptr) == _abi.MIRT_ERR_NO_SCENE
        assert empty.bvh_refits() == 0
    ctx.set_scene(_scene(a))                                        # an LDS scene
    want = ctx.render(_pt())
    assert lib.mirt_ctx_update_spheres(ctx._h, 0, 1, ptr) == _abi.MIRT_ERR_NO_SCENE
    with pytest.raises(m.MirtError) as e:
        ctx.update_spheres(0, a[:1])
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    assert_images_equal(ctx.render(_pt()), want, "an LDS scene after a refused update")
    for b in BUILDERS:
        ctx = ctxs[b]
        ctx.set_scene(_scene(a), hbm=True, bvh=b)
        ctx.update_spheres(0, a[:2])
        assert ctx.bvh_refits() == 1
        want, tree = ctx.render(_pt()), _tree_bytes(ctx)
        for first, count, p, status in ((0, n + 1, ptr, _abi.MIRT_ERR_BAD_ROWS), (n, 1, ptr, _abi.MIRT_ERR_BAD_ROWS), (1, n, ptr, _abi.MIRT_ERR_BAD_ROWS),
                                        (2 ** 32 - 1, 2, ptr, _abi.MIRT_ERR_BAD_ROWS), (0, 1, None, _abi.MIRT_ERR_NULL_POINTER)):
            for fn in (lib.mirt_ctx_update_spheres, lib.mirt_ctx_update_spheres_device):
                assert fn(ctx._h, first, count, p) == status, (first, count)
            assert _tree_bytes(ctx) == tree and ctx.bvh_refits() == 1
            assert_images_equal(ctx.render(_pt()), want, f"after the refused update ({first}, {count})")
        ctx.set_scene(_scene(a), hbm=True, bvh=b)
        assert ctx.bvh_refits() == 0                                # every set_scene* starts the count again


# ---- culling: a refitted tree renders the right bytes however loose it is, so the work is counted ----

COUNT = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID


@pytest.mark.parametrize("b", BUILDERS)
def test_an_update_with_the_same_data_leaves_the_traversal_alone(ctxs, b):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(5000)
    ctx = ctxs[b]
    ctx.set_scene(scene_from_arrays(look(w, h, **FIELD_VIEW), arr, mats, tex), hbm=True, bvh=b)
    p = _pt(w, h, 2, flags=COUNT)
    img, before, tree = ctx.render(p), ctx.stats(), _tree_bytes(ctx)
    ctx.update_spheres(0, arr)
    assert ctx.bvh_refits() == 1 and _tree_bytes(ctx) == tree
    assert_images_equal(ctx.render(p), img, "an update with the scene's own data")
    after = ctx.stats()
    for k in ("rays", "hits", "sphere_tests", "grid_cells", "grid_wave_cells"):
        assert after[k] == before[k], k


# sphere_tests of the refitted tree / sphere_tests of a fresh host tree of the moved world, as measured (the counters are deterministic);
# the test allows 25 % more, which only absorbs later changes of a builder
MEASURED_TESTS_RATIO = {"host": 0.9702, "device": 0.9951}


@pytest.mark.parametrize("b", BUILDERS)
def test_a_refitted_tree_still_culls(ctxs, b):
    """rtiow_field(5000), every small sphere jittered by up to 0.25 of its radius in x and z: sphere_tests against a freshly built
    HOST tree of the moved world.  Measured on an MI355X at 64x48 x 2 spp, fresh host tree 104 894 tests: the refitted host tree
    101 770 (0.9702: the looser boxes visit 2.9 % more nodes, whose leaves happen to hold fewer spheres), the refitted device tree
    104 377 (0.9951, 5.0 % more nodes).  The bound is 1.25 x the measured ratio."""
    w, h = 64, 48
    arr, mats, tex = rtiow_field(5000)
    rng = np.random.default_rng(25)
    moved = arr.copy()
    moved["center"][5:, 0] += (rng.uniform(-0.25, 0.25, len(arr) - 5) * arr["radius"][5:]).astype(np.float32)
    moved["center"][5:, 2] += (rng.uniform(-0.25, 0.25, len(arr) - 5) * arr["radius"][5:]).astype(np.float32)
    cam = look(w, h, **FIELD_VIEW)
    p = _pt(w, h, 2, flags=COUNT)
    ctx, fresh = ctxs[b], ctxs["fresh"]
    ctx.set_scene(scene_from_arrays(cam, arr, mats, tex), hbm=True, bvh=b)
    ctx.update_spheres(5, moved[5:])
    fresh.set_scene(scene_from_arrays(cam, moved, mats, tex), hbm=True)
    img, got = ctx.render(p), ctx.stats()
    assert_images_equal(img, fresh.render(p), "jittered field")
    want = fresh.stats()
    for k in ("rays", "hits", "scatter", "sky_misses"):
        assert got[k] == want[k], k
    ratio = got["sphere_tests"] / want["sphere_tests"]
    print(f"refit culling, {b} tree: sphere_tests {got['sphere_tests']} vs fresh host tree {want['sphere_tests']}: ratio {ratio:.4f}; "
          f"nodes visited ratio {got['grid_cells'] / want['grid_cells']:.4f}")
    assert 0 < ratio <= 1.25 * MEASURED_TESTS_RATIO[b]


# ---- node and the host objects ----

def test_node_loopback(ctxs):
    w, h = 32, 24
    a = _soup(257, seed=357)
    bb = _jitter(a, 10)
    ctxs["fresh"].set_scene(_scene(bb, w, h), hbm=True)
    want = ctxs["fresh"].render(_pt(w, h))
    with m.Node([0, 0]) as node:
        lib, ptr = m.lib(), bb.ctypes.data_as(C.c_void_p)
        assert lib.mirt_node_update_spheres(node._h, 0, 1, ptr) == _abi.MIRT_ERR_NO_SCENE
        node.set_scene(_scene(a, w, h), hbm=True, bvh="device")
        assert lib.mirt_node_update_spheres(node._h, 200, 58, ptr) == _abi.MIRT_ERR_BAD_ROWS
        node.update_spheres(0, bb)
        assert_images_equal(node.render(_pt(w, h)), want, "node of 2 after update_spheres")
        assert [node.context(i).bvh_refits() for i in range(2)] == [1, 1]
        node.set_scene(_scene(a, w, h))                             # an LDS scene on every member
        assert lib.mirt_node_update_spheres(node._h, 0, 1, ptr) == _abi.MIRT_ERR_NO_SCENE
        assert node.render(_pt(w, h)).shape == want.shape           # a refused update leaves the node its scene


def test_raytracer_move_spheres():
    """A world beyond the LDS budget goes to device memory: move_spheres updates it in place and restarts the accumulation; a small
    world is set again.  Either way the frames are those of a Raytracer made from the moved scene."""
    arr = rtiow_field(5000)[0]
    mats = [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))), m.Material.Metal(albedo=m.Texture.new_from_color((0.7, 0.6, 0.5)), fuzz=0.2),
            m.Material.Dielectric(refraction_index=1.5)]
    cam = m.Camera(np.asarray((13, 2, 3), np.float32), np.asarray((-0.96, -0.1, -0.22), np.float32), np.asarray((0, 1, 0), np.float32),
                   m.Angle.degrees(25.0), 0.0, 10.0)
    rp = m.RenderParams(camera=cam, sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=2, num_bounces=4), viewport_size=(32, 24))
    for n, in_place in ((5000, True), (40, False)):
        spheres = [m.Sphere(arr["center"][i, :3], float(arr["radius"][i]), int(arr["material_idx"][i]) % 3) for i in range(n)]
        new = [m.Sphere(s.center + np.float32(0.05), s.radius * 1.1, 99) for s in spheres[7:30]]
        rt = m.Raytracer(m.Scene(spheres, mats), rp)
        try:
            rt.render_frame()
            rt.move_spheres(7, new)
            assert rt.progress() == 0.0
            assert rt._ctx.bvh_refits() == (1 if in_place else 0)
            got = [rt.render_frame(), rt.render_frame()]
        finally:
            rt.close()
        moved = spheres[:7] + [m.Sphere(s.center, s.radius, o.material_idx) for s, o in zip(new, spheres[7:30])] + spheres[30:]
        rt = m.Raytracer(m.Scene(moved, mats), rp)
        try:
            rt.render_frame()                                        # the moved Raytracer's frames are numbered from 2 (reference_stream off: no effect)
            rt.set_render_params(rp)
            for i in range(2):
                assert_images_equal(got[i], rt.render_frame(), f"n = {n}: frame {i} after move_spheres")
        finally:
            rt.close()


def test_layer_move_spheres(ctxs):
    """Layer.move_spheres on a world in device memory: updated in place, rendered again; the image is a fresh Layer's of the moved world."""
    arr = rtiow_field(5000)[0]
    mats = [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))), m.Material.Metal(albedo=m.Texture.new_from_color((0.7, 0.6, 0.5)), fuzz=0.2),
            m.Material.Lambertian(albedo=m.Texture.new_from_color((0.8, 0.3, 0.2)))]         # parity mode reads material 2's texture on every hit
    cam = m.Camera(np.asarray((13, 2, 3), np.float32), np.asarray((-0.96, -0.1, -0.22), np.float32), np.asarray((0, 1, 0), np.float32),
                   m.Angle.degrees(25.0), 0.0, 10.0)
    rp = m.RenderParams(camera=cam, viewport_size=(32, 24))
    spheres = [m.Sphere(arr["center"][i, :3], float(arr["radius"][i]), int(arr["material_idx"][i]) % 3) for i in range(len(arr))]
    new = [m.Sphere(s.center + np.float32(0.05), s.radius * 1.5, 99) for s in spheres[1:40]]
    layer = m.Layer.new([32, 24], rp, scene=m.Scene(spheres, mats))
    moved = m.Layer.new([32, 24], rp, scene=m.Scene(spheres[:1] + [m.Sphere(s.center, s.radius, o.material_idx) for s, o in zip(new, spheres[1:40])] + spheres[40:], mats))
    try:
        for la in (layer, moved):
            la.set_global_data()
            la.set_data(rp)
        assert not np.array_equal(layer.register_texture(), moved.register_texture())
        layer.move_spheres(np.int64(1), new, rp)
        assert layer._ctx.bvh_refits() == 1
        assert_images_equal(layer.register_texture(), moved.register_texture(), "Layer.move_spheres vs a Layer of the moved world")
    finally:
        layer.close()
        moved.close()


@pytest.mark.parametrize("n, refits", [(5000, 1), (40, 0)])
def test_cpp_move_spheres(n, refits):
    """The C++ mirror's Raytracer::move_spheres and Layer::move_spheres (host/move_demo.cpp compares each with an object made from the
    moved scene): in place for a world in device memory, by set_scene for a small one."""
    import subprocess
    from pathlib import Path
    host = Path(__file__).resolve().parent.parent / "weekend-raytracer-wgpu_amd" / "host"
    subprocess.run(["make", "-C", str(host)], check=True, capture_output=True)
    r = subprocess.run([str(host / "move_demo"), str(n), "48", "32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.splitlines() == [f"raytracer: equal refits {refits}", f"layer: equal refits {refits}", "layer range: MIRT_ERR_BAD_ROWS world kept"]
