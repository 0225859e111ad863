"""mirt_bvh_plan: the BVH mirt_ctx_set_scene_ex(MIRT_SCENE_HBM) builds, host only (no GPU)."""
import ctypes as C
import time

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from hbm_worlds import c_spheres, clustered_soup, rtiow_field, sphere_array
import deep_worlds


def _plan(arr):
    carr, keep = c_spheres(arr)
    return m.bvh_plan(carr)


def _soup(n, seed=0):
    rng = np.random.default_rng(seed)
    return sphere_array(rng.uniform(-50, 50, (n, 3)), rng.uniform(0.1, 1.0, n), np.zeros(n))


def _rtiow():
    sc, _ = m.scenes.rtiow_final()
    sph = [s.to_c() for s in sc.spheres]
    return sphere_array([list(s.center)[:3] for s in sph], [s.radius for s in sph], [s.material_idx for s in sph])


def _inputs():
    rng = np.random.default_rng(3)
    yield "rtiow", _rtiow()
    for n in (1, 2, 31, 32, 1000, 100000):
        yield f"soup{n}", _soup(n, n)
    yield "identical", sphere_array(np.tile([[1.0, 2.0, 3.0]], (10000, 1)), np.full(10000, 0.5), np.zeros(10000))
    t = np.arange(10000, dtype=np.float64)
    yield "line", sphere_array(np.stack([t * 0.1, t * 0, t * 0], 1), np.full(10000, 0.04), np.zeros(10000))
    shells = np.concatenate([np.zeros((200, 3)), rng.normal(0, 0.01, (200, 3))])
    yield "shells", sphere_array(shells, np.concatenate([np.linspace(0.1, 20, 200), np.linspace(0.01, 0.5, 200)]), np.zeros(400))
    yield "radii1e6", sphere_array(rng.uniform(-100, 100, (3000, 3)), 10.0 ** rng.uniform(-3, 3, 3000), np.zeros(3000))
    neg = _soup(2000, 4)
    neg["radius"][::3] *= -1
    yield "negative", neg
    bad = _soup(500, 5)
    bad["center"][7, 0] = np.inf
    yield "nonfinite", bad
    yield "field", rtiow_field(20000)[0]
    yield "clustered", clustered_soup(20000)[0]
    yield "line26", deep_worlds.line("line26")
    yield "line32", deep_worlds.line("line32")


INPUTS = list(_inputs())


@pytest.mark.parametrize("case", range(len(INPUTS)), ids=[name for name, _ in INPUTS])
def test_plan_invariants(case):
    name, arr = INPUTS[case]
    n = len(arr)
    p = _plan(arr)
    assert p["max_depth"] <= _abi.MIRT_BVH_MAX_DEPTH
    assert 1 <= p["max_leaf"] <= _abi.MIRT_BVH_MAX_LEAF
    assert p["n_leaf_spheres"] + p["n_always"] == n
    assert p["n_always"] <= _abi.MIRT_BVH_MAX_ALWAYS
    assert p["n_nodes"] == p["n_leaves"] - 1
    assert p["n_leaves"] * _abi.MIRT_BVH_MAX_LEAF >= p["n_leaf_spheres"]
    assert p["device_bytes"] == 64 * p["n_nodes"] + 20 * n
    assert _plan(arr.copy()) == p, "not deterministic"


def test_big_and_nonfinite_spheres_go_to_the_always_list():
    assert _plan(_rtiow())["n_always"] == 4                    # the ground sphere and the three r = 1 heroes (> 4 x 0.2)
    bad = _soup(500, 5)
    bad["center"][7, 0] = np.inf
    bad["radius"][9] = np.nan
    assert _plan(bad)["n_always"] == 2


def test_identical_spheres_build_median_trees():
    p = _plan(sphere_array(np.tile([[1.0, 2.0, 3.0]], (10000, 1)), np.full(10000, 0.5), np.zeros(10000)))
    assert p["max_depth"] == 12                                # ceil(log2(10000 / 4))
    assert p["max_leaf"] == 4


def test_limits_and_errors():
    out = _abi.MirtBvhPlan()
    too_many = _abi.MIRT_SCENE_HBM_MAX_SPHERES + 1
    assert m.lib().mirt_bvh_plan(C.c_void_p(16), too_many, C.byref(out)) == _abi.MIRT_ERR_SCENE_TOO_LARGE   # refused before a read
    assert m.lib().mirt_bvh_plan(None, 5, C.byref(out)) == _abi.MIRT_ERR_NULL_POINTER
    assert m.bvh_plan([]) == dict(n_nodes=0, n_leaves=0, n_leaf_spheres=0, n_always=0, max_depth=0, max_leaf=0, device_bytes=0)


def test_million_sphere_field_plans_in_ten_seconds():
    arr = rtiow_field(1000000, seed=7)[0]
    t0 = time.perf_counter()
    p = _plan(arr)
    dt = time.perf_counter() - t0
    print(f"1M-sphere field: planned in {dt:.2f} s: {p}")
    assert dt <= 10.0
    assert p["max_depth"] <= _abi.MIRT_BVH_MAX_DEPTH and p["n_leaf_spheres"] + p["n_always"] == 1000000
