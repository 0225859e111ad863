"""MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE: the BVH of an HBM scene built on the device.

The tree is a different one from the host's (Morton order instead of binned SAH), so nothing here compares trees.  What must hold:
the tree has the properties the exactness argument of DESIGN.md 10.1 needs (tests/bvh_check.py, on worlds at every boundary of the
builder), it is a pure function of the input, the image is the host tree's / the LDS builds' / the flat scan's byte for byte, and the
tree still culls (a loose tree renders the right bytes too: that is counted separately)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from bvh_check import check_bvh
from helpers import assert_images_equal, bimodal_soup, scene_data
from hbm_worlds import clustered_soup, field_materials, look, rtiow_field, scene_from_arrays, sphere_array

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
DEV = dict(hbm=True, bvh="device")
HBM_DEVICE = _abi.MIRT_SCENE_HBM | _abi.MIRT_SCENE_BVH_DEVICE
BVH_KERNEL = "render_pt_hbm_kernel<false,false,true,true>"
_MATS = []


def _mats():
    if not _MATS:
        _MATS.append(field_materials())
    return _MATS[0]


def _pt(w, h, spp, **kw):
    kw.setdefault("num_bounces", 8)
    return m.make_params(w, h, spp, mode=PT, **kw)


@pytest.fixture(scope="module")
def dctx():
    ctx = m.Context(0)
    yield ctx
    ctx.close()


def _scene(arr, w=16, h=16, eye=(0, 0.5, 4), at=(0, 0, -6), vfov=50):
    mats, tex = _mats()
    return scene_from_arrays(look(w, h, eye, at, vfov=vfov), arr, mats, tex)


def _soup(n, seed):
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-4, 4, (n, 3))
    cen[:, 2] -= 6
    rad = rng.uniform(0.05, 0.6, n) * (1.0 if n < 200 else 0.4)
    return sphere_array(cen, rad, rng.integers(0, len(_mats()[0]), n))


def _validate(ctx, arr):
    """Builds `arr` on the device and runs the validator on what the context holds -> (the walk's counts, info)."""
    ctx.set_scene(_scene(arr), **DEV)
    info = ctx.bvh_info()
    assert info["built_on_device"] == 1
    nodes, recs, ids = ctx.bvh_read()
    count = check_bvh(nodes, recs, ids, info, arr["center"][:, :3], arr["radius"])
    assert count["n_leaf_spheres"] + count["n_always"] == len(arr)
    return count, info


# ---- 1. structure: the device tree passes the validator at every boundary of the builder ----

@pytest.mark.parametrize("n", [0, 1, 4, 5, 8, 9, 63, 64, 65, 257, 1025])
def test_structure_of_seeded_soups(dctx, n):
    """Leaf / first inner node / wave / block boundaries of the level kernels."""
    count, info = _validate(dctx, _soup(n, seed=100 + n))
    assert count["n_nodes"] == (0 if n <= 4 else count["n_leaves"] - 1)
    assert bool(info["root"] & m.BVH_LEAF) == (n <= 4)


@pytest.mark.parametrize("world", ["field5000", "clusters20000"])
def test_structure_of_large_worlds(dctx, world):
    arr = rtiow_field(5000)[0] if world == "field5000" else clustered_soup(20000)[0]
    count, _ = _validate(dctx, arr)
    if world == "field5000":
        assert count["n_always"] == 5                 # the ground and the four heroes (|r| = 1, 0.9, 1, 1), as on the host


def test_structure_of_identical_spheres(dctx):
    """1 000 copies of one sphere: all codes are equal, every split is a median split, 250 leaves of 4 at depth 8."""
    n = 1000
    arr = sphere_array(np.tile([[0.0, 0.0, -3.0]], (n, 1)), np.full(n, 0.7), np.arange(n) % 7)
    count, _ = _validate(dctx, arr)
    assert count["max_depth"] == 8 and count["n_always"] == 0


def test_structure_of_a_planar_world(dctx):
    """Every centre at y = 0, equal radii: the centroid box has no extent on that axis (cell 0 there, never a division by it)."""
    rng = np.random.default_rng(11)
    n = 600
    cen = np.stack([rng.uniform(-20, 20, n), np.zeros(n), rng.uniform(-30, -5, n)], 1)
    _validate(dctx, sphere_array(cen, np.full(n, 0.25), rng.integers(0, 7, n)))


def test_structure_with_seventy_non_finite_spheres(dctx):
    """64 of them fill the always-tested list, 6 stay in the tree with infinite boxes (and centre 0 for the keys)."""
    rng = np.random.default_rng(12)
    n = 570
    cen = rng.uniform(-4, 4, (n, 3))
    rad = rng.uniform(0.1, 0.3, n)
    bad = np.sort(rng.choice(n, 70, replace=False))
    for j, i in enumerate(bad):
        if j % 4 == 0: cen[i, j % 3] = np.inf
        elif j % 4 == 1: cen[i, j % 3] = np.nan
        elif j % 4 == 2: rad[i] = np.inf
        else: rad[i] = np.nan
    arr = sphere_array(cen, rad, rng.integers(0, 7, n))
    count, info = _validate(dctx, arr)
    assert count["n_always"] == 64 and count["n_leaf_spheres"] == n - 64
    nodes, _, ids = dctx.bvh_read()
    assert ids[:64].tolist() == bad[:64].tolist()
    assert info["radius"] == float(np.float32(3.0e38))           # an infinite box in the tree: the bound is the clamp
    assert np.isinf(nodes["lmin"]).any() and np.isinf(nodes["rmax"]).any()


def test_structure_with_centres_at_1e37(dctx):
    rng = np.random.default_rng(13)
    n = 300
    cen = rng.choice([-1.0e37, 1.0e37], (n, 3)) + rng.uniform(-1e36, 1e36, (n, 3))
    count, info = _validate(dctx, sphere_array(cen, np.full(n, 1.0e35), rng.integers(0, 7, n)))
    assert np.isfinite(info["radius"]) and info["radius"] < 3.0e38


def _staircase():
    """For k = 1 .. 24 and each axis a, five spheres of radius 2^-(k+4) within 2^-(k+3) of 2^-k e_a, and five at the origin: 365
    spheres whose Morton codes peel one group per level for 3 x (bits per axis) levels."""
    rng = np.random.default_rng(14)
    cen, rad = [], []
    for k in range(1, 25):
        for a in range(3):
            base = np.zeros(3)
            base[a] = 2.0 ** -k
            cen.append(base + rng.uniform(-1, 1, (5, 3)) * 2.0 ** -(k + 4))         # |offset| <= sqrt(3) 2^-(k+4) < 2^-(k+3)
            rad.append(np.full(5, 2.0 ** -(k + 4)))
    cen.append(rng.uniform(-1, 1, (5, 3)) * 2.0 ** -29)
    rad.append(np.full(5, 2.0 ** -29))
    cen, rad = np.concatenate(cen), np.concatenate(rad)
    assert len(rad) == 365
    return sphere_array(cen, rad, np.arange(365) % 7)


def test_structure_of_the_axes_staircase(dctx):
    """With >= 11 code bits per axis the Morton splits alone would go deeper than 32: only the depth rule keeps the invariant."""
    count, _ = _validate(dctx, _staircase())
    assert count["max_depth"] <= m.MIRT_BVH_MAX_DEPTH


def _aligned_staircase():
    """The staircase with everything the builder's choices could soften taken away: equal radii (nothing goes to the always-tested
    list), offsets towards +x +y +z only and one centre at the origin (the centroid box starts at 0, so group k on axis a keeps the
    top bit of its cell to itself whatever the code width and the cells' shape).  Pure Morton splits peel one group per level: replayed
    in numpy they reach depth 36 / 39 / 45 / 53 / 67 with 10 / 11 / 13 / 16 / 21 bits per axis; with the depth rule, 32."""
    rng = np.random.default_rng(15)
    cen = []
    for k in range(1, 25):
        for a in range(3):
            base = np.zeros(3)
            base[a] = 2.0 ** -k
            cen.append(base + rng.uniform(0, 1, (5, 3)) * 2.0 ** -(k + 4))
    origin = rng.uniform(0, 1, (5, 3)) * 2.0 ** -29
    origin[0] = 0.0
    cen = np.concatenate(cen + [origin])
    return sphere_array(cen, np.full(len(cen), 2.0 ** -30), np.arange(len(cen)) % 7)


def test_structure_of_the_aligned_staircase(dctx):
    count, _ = _validate(dctx, _aligned_staircase())
    assert count["n_always"] == 0 and count["max_depth"] <= m.MIRT_BVH_MAX_DEPTH


# ---- 2. determinism ----

def test_two_builds_give_the_same_bytes(dctx):
    arr = clustered_soup(20000)[0]
    sd = _scene(arr)
    dctx.set_scene(sd, **DEV)
    first = [a.tobytes() for a in dctx.bvh_read()]
    info = dctx.bvh_info()
    dctx.set_scene(_scene(_soup(3000, 3)), **DEV)                 # another world in between: the scratch is dirty
    dctx.set_scene(sd, **DEV)
    assert [a.tobytes() for a in dctx.bvh_read()] == first
    assert dctx.bvh_info() == info
    with m.Context(0) as other:                                   # and on a fresh context
        other.set_scene(sd, **DEV)
        assert [a.tobytes() for a in other.bvh_read()] == first


# ---- 3. images: byte-equal to the host tree, the LDS builds, the oracle, the flat scan ----

def _lds_scenes(w, h):
    out = [(name, scene_data(name, w, h)) for name in ("three_spheres", "main_rs_scene", "earth", "rtiow_final")]
    cs, rs = bimodal_soup()
    mats, tex = _mats()
    rng = np.random.default_rng(5)
    arr = sphere_array(cs, rs, rng.integers(0, len(mats), len(rs)))
    out.append(("bimodal_soup", scene_from_arrays(look(w, h, (0, 0, 3), (0, 0, 0), vfov=40), arr, mats, tex)))
    for n, seed in ((32, 1), (500, 2), (3000, 3)):
        out.append((f"soup{n}", scene_from_arrays(look(w, h, (0, 0.5, 4), (0, 0, -6), vfov=50), _soup(n, seed), mats, tex)))
    return out


BUILDS = (("lds", {}), ("host tree", dict(hbm=True)), ("device tree", DEV))


def test_images_and_sums_equal_the_host_tree_and_the_lds_builds(dctx):
    w, h = 64, 40
    for name, sd in _lds_scenes(w, h):
        images, sums = {}, {}
        for build, kw in BUILDS:
            dctx.set_scene(sd, **kw)
            images[build] = [dctx.render(_pt(w, h, spp)) for spp in (1, 2, 8, 32)]
            if kw:
                assert dctx.last_kernel() == BVH_KERNEL, dctx.last_kernel()
            p = _pt(w, h, 4)
            dctx.accum_reset(p)
            dctx.accum_add(p)
            sums[build] = dctx.accum_read(p)
        for other in ("host tree", "lds"):
            for i, spp in enumerate((1, 2, 8, 32)):
                assert_images_equal(images["device tree"][i], images[other][i], f"{name} spp{spp}: device tree vs {other}")
            assert np.array_equal(sums["device tree"], sums[other]), f"{name}: accumulated sums differ from the {other}'s"


def test_accum_frame_and_frame_spp(dctx):
    w, h = 64, 40
    sd = _lds_scenes(w, h)[6][1]                                  # soup500
    got = {}
    for build, kw in BUILDS[1:]:
        dctx.set_scene(sd, **kw)
        p = _pt(w, h, 4)
        dctx.accum_reset(p)
        frames = [dctx.accum_frame(p), dctx.accum_frame(p)]
        got[build] = (frames, dctx.accum_read(p), dctx.render(_pt(w, h, 8, frame_spp=2, frame_begin=3)))
    for i in range(2):
        assert_images_equal(got["device tree"][0][i], got["host tree"][0][i], f"mirt_ctx_accum_frame {i}")
    assert np.array_equal(got["device tree"][1], got["host tree"][1])
    assert_images_equal(got["device tree"][2], got["host tree"][2], "frame_spp = 2")


def test_field_of_5000_against_the_oracle(dctx, oracle):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(5000)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=25, aperture=0.05), arr, mats, tex)
    p = _pt(w, h, 4, num_bounces=6)
    dctx.set_scene(sd, **DEV)
    assert_images_equal(dctx.render(p), oracle.render(sd, p), "field 5 000: device tree vs oracle")


def test_field_of_100000_against_the_device_flat_scan(dctx):
    w, h = 256, 144
    arr, mats, tex = rtiow_field(100000, seed=100000)
    sd = scene_from_arrays(look(w, h, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    dctx.set_scene(sd, **DEV)
    got = dctx.render(_pt(w, h, 8, num_bounces=4))
    assert dctx.last_kernel() == BVH_KERNEL
    flat = dctx.render(_pt(w, h, 8, num_bounces=4, flags=m.MIRT_FLAG_NO_GRID))
    assert dctx.last_kernel().startswith("render_pt_hbm_kernel<false,false,false,")
    assert_images_equal(got, flat, "100 000 spheres: device tree vs flat scan")


def _adversarial():
    """The adversarial worlds of test_gpu_hbm_scene.py: 1 000 copies of one sphere, a tangent 13^3 lattice seen along an axis and
    obliquely, a camera inside a big sphere, rays grazing r = 1e-3 spheres at distance 1e3 with zero-radius and non-finite ones."""
    from grid_rounding import adversarial_worlds
    return [(name, sphere_array(cen, rad, mat), eye, at, vfov) for name, cen, rad, mat, eye, at, vfov in adversarial_worlds(lattice_half=6)]


@pytest.mark.parametrize("case", range(5))
def test_adversarial_geometry_against_the_flat_scan(dctx, case):
    name, arr, eye, at, vfov = _adversarial()[case]
    w, h = 48, 32
    dctx.set_scene(_scene(arr, w, h, eye, at, vfov), **DEV)
    got = dctx.render(_pt(w, h, 4, num_bounces=5))
    assert dctx.last_kernel() == BVH_KERNEL
    assert_images_equal(got, dctx.render(_pt(w, h, 4, num_bounces=5, flags=m.MIRT_FLAG_NO_GRID)), f"{name}: device tree vs flat scan")


def test_a_million_spheres(dctx):
    w, h = 128, 72
    arr, mats, tex = rtiow_field(1000000, seed=7)
    sd = scene_from_arrays(look(w, h, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    dctx.set_scene(sd, **DEV)
    info = dctx.bvh_info()
    plan = info["plan"]
    assert info["built_on_device"] == 1
    assert plan["n_leaf_spheres"] + plan["n_always"] == len(arr) and plan["n_always"] == 5
    assert plan["max_depth"] <= m.MIRT_BVH_MAX_DEPTH and 1 <= plan["max_leaf"] <= _abi.MIRT_BVH_MAX_LEAF
    assert plan["n_leaves"] == plan["n_nodes"] + 1 and plan["device_bytes"] == 64 * plan["n_nodes"] + 20 * len(arr)
    p = _pt(w, h, 2, num_bounces=4, row_begin=24, row_end=48)
    got = dctx.render(p)
    assert dctx.last_kernel() == BVH_KERNEL
    dctx.set_scene(sd, hbm=True)
    assert dctx.bvh_info()["built_on_device"] == 0
    assert_images_equal(got, dctx.render(p), "1 000 000 spheres: device tree vs host tree")


# ---- 4. culling: a loose tree renders the right bytes too, so the work is counted ----

@pytest.mark.parametrize("world", ["field5000", "clusters20000"])
def test_the_device_tree_culls(dctx, world):
    """sphere_tests and nodes visited of the device tree <= 4 x the host tree's.  A condition, not a performance claim: a tree that
    does not cull costs hundreds of times the host tree's counts on these worlds."""
    w, h = 64, 48
    if world == "field5000":
        arr, mats, tex = rtiow_field(5000)
        cam = look(w, h, (13, 2, 3), (0, 0, 0), vfov=25)
    else:
        arr, mats, tex = clustered_soup(20000)
        cam = look(w, h, (0, 5, 60), (0, 0, 0), vfov=60)
    sd = scene_from_arrays(cam, arr, mats, tex)
    p = _pt(w, h, 4, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID)
    stats, images = {}, {}
    for build, kw in BUILDS[1:]:
        dctx.set_scene(sd, **kw)
        images[build] = dctx.render(p)
        stats[build] = dctx.stats()
    assert_images_equal(images["device tree"], images["host tree"], world)
    for k in ("rays", "hits", "scatter", "sky_misses"):
        assert stats["device tree"][k] == stats["host tree"][k], k
    for k in ("sphere_tests", "grid_cells"):
        print(f"{world}: {k} device tree {stats['device tree'][k]} host tree {stats['host tree'][k]} "
              f"ratio {stats['device tree'][k] / stats['host tree'][k]:.3f}")
        assert 0 < stats["device tree"][k] <= 4 * stats["host tree"][k], k


# ---- 5. flags and errors ----

def test_flags_and_errors(dctx):
    w, h = 48, 32
    sd = scene_data("rtiow_final", w, h)
    lib, c = m.lib(), sd.as_c()
    dctx.set_scene(sd, hbm=True)
    want = dctx.render(_pt(w, h, 4))
    for flags in (_abi.MIRT_SCENE_BVH_DEVICE, _abi.MIRT_SCENE_HBM | 4, HBM_DEVICE | 4):
        assert lib.mirt_ctx_set_scene_ex(dctx._h, C.byref(c), flags) == _abi.MIRT_ERR_BAD_MODE, flags
    assert_images_equal(dctx.render(_pt(w, h, 4)), want, "after refused calls")
    with pytest.raises(ValueError):
        dctx.set_scene(sd, bvh="device")
    # for a host-built tree, bvh_info.plan == mirt_bvh_plan
    info = dctx.bvh_info()
    assert info["built_on_device"] == 0 and info["plan"] == m.bvh_plan(list(sd.spheres))
    arr = rtiow_field(5000)[0]
    dctx.set_scene(_scene(arr), hbm=True)
    from hbm_worlds import c_spheres
    assert dctx.bvh_info()["plan"] == m.bvh_plan(c_spheres(arr)[0])
    nodes, recs, ids = dctx.bvh_read()
    check_bvh(nodes, recs, ids, dctx.bvh_info(), arr["center"][:, :3], arr["radius"])          # the host tree passes the validator too
    # the accepted flag builds; short buffers are refused
    assert lib.mirt_ctx_set_scene_ex(dctx._h, C.byref(c), HBM_DEVICE) == 0, lib.mirt_last_error()
    assert_images_equal(dctx.render(_pt(w, h, 4)), want, "HBM | BVH_DEVICE")
    plan = dctx.bvh_info()["plan"]
    n = plan["n_leaf_spheres"] + plan["n_always"]
    nodes, recs, ids = np.zeros(plan["n_nodes"] * 64, np.uint8), np.zeros(4 * n, np.float32), np.zeros(n, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mirt_ctx_bvh_read(dctx._h, ptr(nodes), nodes.nbytes, ptr(recs), recs.size, ptr(ids), ids.size) == 0
    assert lib.mirt_ctx_bvh_read(dctx._h, ptr(nodes), nodes.nbytes - 1, ptr(recs), recs.size, ptr(ids), ids.size) == _abi.MIRT_ERR_OUT_BUFFER
    assert lib.mirt_ctx_bvh_read(dctx._h, ptr(nodes), nodes.nbytes, ptr(recs), recs.size - 1, ptr(ids), ids.size) == _abi.MIRT_ERR_OUT_BUFFER
    assert lib.mirt_ctx_bvh_read(dctx._h, ptr(nodes), nodes.nbytes, ptr(recs), recs.size, ptr(ids), ids.size - 1) == _abi.MIRT_ERR_OUT_BUFFER
    # bvh_info / bvh_read without an HBM scene
    out = _abi.MirtBvhInfo()
    dctx.set_scene(sd)
    assert lib.mirt_ctx_bvh_info(dctx._h, C.byref(out)) == _abi.MIRT_ERR_NO_SCENE
    assert lib.mirt_ctx_bvh_read(dctx._h, ptr(nodes), nodes.nbytes, ptr(recs), recs.size, ptr(ids), ids.size) == _abi.MIRT_ERR_NO_SCENE
    with m.Context(0) as fresh:
        assert lib.mirt_ctx_bvh_info(fresh._h, C.byref(out)) == _abi.MIRT_ERR_NO_SCENE


# ---- 6. node: every member builds its own tree ----

@pytest.mark.parametrize("members", [2, 4])
def test_node_loopback(dctx, members):
    w, h = 64, 40
    arr, mats, tex = rtiow_field(8000, seed=8)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    dctx.set_scene(sd, **DEV)
    want = dctx.render(_pt(w, h, 4))
    node = m.Node([0] * members)
    try:
        c = sd.as_c()
        for flags in (_abi.MIRT_SCENE_BVH_DEVICE, HBM_DEVICE | 4):
            assert m.lib().mirt_node_set_scene_ex(node._h, C.byref(c), flags) == _abi.MIRT_ERR_BAD_MODE
        node.set_scene(sd, **DEV)
        assert_images_equal(node.render(_pt(w, h, 4)), want, f"node of {members}")
        for i in range(members):
            assert node.context(i).bvh_info()["built_on_device"] == 1
    finally:
        node.close()
