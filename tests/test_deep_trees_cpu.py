"""The deep-tree fixtures (tests/deep_worlds.py) and the numpy walk (tests/bvh_walk_ref.py) without a GPU: the host builder's depths
land where the pooled kernel changes its geometry, and on a hand-assembled 32-level tree the walk returns the flat scan's records
with a stack of 32 entries and different ones with 31 -- which is what lets the device comparison of tests/test_gpu_deep_trees.py
fail."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from bvh_check import assemble, check_bvh
from bvh_walk_ref import walk
from hbm_worlds import c_spheres
import deep_worlds as dw
import ray_query_ref as rq


@pytest.mark.parametrize("name", list(dw.LINES))
def test_host_depths_select_every_pooled_geometry(name):
    lo, hi = dw.TARGETS[name]
    plan = m.bvh_plan(c_spheres(dw.line(name))[0])
    print(f"{name}: {plan}")
    assert lo <= plan["max_depth"] <= hi and plan["n_always"] == 0
    for depth in range(lo, hi + 1):
        pool = m.bvh_pool_plan(depth)
        assert (pool["slots"], pool["waves_per_cu"]) == dw.pool_geometry(depth) and pool["stack_entries"] == depth, (depth, pool)
    assert dw.pool_geometry(plan["max_depth"]) == {"line22": (80, 16), "line24": (64, 16), "line26": (112, 12), "line32": (96, 12)}[name]


def test_line32_is_exactly_as_deep_as_the_strip_kernels_stack():
    assert m.bvh_plan(c_spheres(dw.line("line32"))[0])["max_depth"] == 32 == m.MIRT_BVH_MAX_DEPTH
    assert m.bvh_pool_plan(32)["lds_bytes_per_block"] == 96 + 4 * (50 * 96 + 384 + 256 * 32)         # 32 KB of stacks per block


@pytest.fixture(scope="module")
def caterpillar_tree():
    arr, topology = dw.caterpillar()
    cen, rad = rq.world_arrays(arr)
    tree = assemble(topology, cen, rad)
    count = check_bvh(*tree, cen, rad)
    assert count["max_depth"] == 32 and count["n_nodes"] == 32 and count["n_always"] == 0
    return tree, rad


def test_the_walk_on_a_32_level_caterpillar(caterpillar_tree):
    tree, rad = caterpillar_tree
    _, o, d = dw.ray_set("caterpillar")
    want = dw.reference("caterpillar")
    got, high, dropped = walk(*tree, o, d, dw.T_MAX, 32, rad)
    same = rq.same_bits(got, want)
    print(f"cap 32: {int((~same).sum())} records differ, {int(dropped.sum())} pushes dropped, high water 32 on {int((high == 32).sum())} rays")
    assert same.all(), f"ray {np.nonzero(~same)[0][0]}"
    assert dropped.sum() == 0 and high.max() == 32 and (high == 32).sum() >= 16
    got, high, dropped = walk(*tree, o, d, dw.T_MAX, 31, rad)
    differ = ~rq.same_bits(got, want)
    print(f"cap 31: {int(differ.sum())} records differ, {int((dropped > 0).sum())} rays drop a push")
    assert high.max() == 31 and (dropped > 0).sum() >= 16 and differ.sum() >= 16
    assert not differ[dropped == 0].any()                            # a ray that dropped nothing walked the same walk


def test_a_bound_on_the_ray_prunes_without_changing_the_answer(caterpillar_tree):
    """closest0 = t_max: with the bound just above / at the winner's root the walk gives resolve()'s strict answer."""
    tree, rad = caterpillar_tree
    arr, o, d = dw.ray_set("caterpillar")
    ref = dw.reference("caterpillar")
    hit = ref["sphere"] != rq.MISS
    t = np.where(hit, ref["t"], np.float32(1.0)).astype(np.float32)
    cen, radii = rq.world_arrays(arr)
    for t_max in (np.nextafter(t, np.float32(np.inf)), t):
        got, _, dropped = walk(*tree, o[::8], d[::8], t_max[::8], 32, rad)
        assert rq.same_bits(got, rq.trace_ref(o[::8], d[::8], t_max[::8], cen, radii)).all() and dropped.sum() == 0


@pytest.mark.parametrize("name", list(dw.LINES) + list(dw.STAIRS) + ["caterpillar"])
def test_sets_are_not_trivial(name):
    arr, o, d = dw.ray_set(name)
    assert len(o) <= 4096 and o.dtype == d.dtype == np.float32
    hits = (dw.reference(name)["sphere"] != rq.MISS).mean()
    print(f"{name}: {len(arr)} spheres, {len(o)} rays, {100 * hits:.1f} % hits")
    assert 0.20 <= hits <= 0.95
    assert np.isfinite(arr["radius"] * arr["radius"]).all() and (arr["radius"] * arr["radius"] >= np.finfo(np.float32).tiny).all()


def test_the_staircase_stays_off_the_always_list():
    plan = m.bvh_plan(c_spheres(dw.axes_staircase())[0])
    assert plan["n_always"] == 0 and plan["n_leaf_spheres"] == 365


@pytest.mark.parametrize("name", list(dw.LINES) + list(dw.STAIRS))
def test_the_host_builders_depth_of_every_world(name):
    assert m.bvh_plan(c_spheres(dw.ray_set(name)[0])[0])["max_depth"] == dw.HOST_DEPTH[name]


def test_an_unknown_set_is_an_error():
    with pytest.raises(KeyError):
        dw.ray_set("staircase")


@pytest.mark.parametrize("name", list(dw.LINES))
def test_the_lds_grid_plan_survives_an_extent_of_2_to_the_83_cells(name):
    """These worlds fit LDS, and their LDS build is a witness of the deep-tree tests.  At the default cell (2.5 median radii = 2^-27.7)
    line32 is 2^83 cells long: build_grid converted that count to uint32 before it compared it with the limit -- undefined, 0 in
    practice -- took the grid of no cells for one that fits, and wrote into its first list (a segmentation fault in
    mirt_ctx_set_scene and mirt_grid_plan)."""
    import grid_rounding as gr
    from hbm_worlds import field_materials, scene_from_arrays
    mats, tex = field_materials()
    sd = scene_from_arrays(dw.line_camera(48, 32), dw.line(name), mats, tex)
    plan = gr.grid_plan(sd)
    print(f"{name}: {[(f, getattr(plan, f)) for f, _ in plan._fields_]}")
    assert 1 <= plan.n_cells <= gr.GRID_MAX_CELLS and plan.n_big == 0
    assert len(dw.line(name)) <= plan.n_entries <= 65535                   # every sphere is listed somewhere
    b = gr.binning(*gr.spheres_of(sd), cell_factor=plan.cell_factor)       # the numpy restatement settles on the same grid
    assert int(np.prod(b["dims"])) == plan.n_cells and b["n_entries"] == plan.n_entries
