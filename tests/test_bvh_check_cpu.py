"""tests/bvh_check.py on hand-made trees: a correct tree passes, and each single defect the validator exists for is refused."""
import numpy as np
import pytest

from bvh_check import LEAF, NODE_DTYPE, BvhError, always_list, assemble, check_bvh, sphere_boxes


def _world(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-5, 5, (n, 3)).astype(np.float32), rng.uniform(0.1, 0.3, n).astype(np.float32)


def _two_leaves():
    cen, rad = _world(8)
    return (*assemble(([0, 1, 2, 3], [4, 5, 6, 7]), cen, rad), cen, rad)


def test_a_correct_two_leaf_tree_passes():
    count = check_bvh(*_two_leaves())
    assert count == {"n_nodes": 1, "n_leaves": 2, "n_leaf_spheres": 8, "n_always": 0, "max_depth": 1, "max_leaf": 4}


def test_an_empty_tree_and_a_single_leaf_pass():
    cen, rad = _world(3)
    count = check_bvh(*assemble([], cen[:0], rad[:0]), cen[:0], rad[:0])
    assert count["n_leaves"] == 0 and count["n_nodes"] == 0
    assert check_bvh(*assemble([0, 1, 2], cen, rad), cen, rad)["max_depth"] == 0


def test_a_correct_tree_with_an_always_list_and_three_levels_passes():
    cen, rad = _world(12, seed=1)
    rad[5] = 100.0                                   # above 4 median radii: the host rule puts it on the list
    assert always_list(cen, rad).tolist() == [5]
    rest = [i for i in range(12) if i != 5]
    check_bvh(*assemble(((rest[:3], rest[3:6]), (rest[6:8], rest[8:])), cen, rad, always=[5]), cen, rad)
    with pytest.raises(BvhError, match="always-tested list"):
        check_bvh(*assemble(((list(range(3)), list(range(3, 6))), (list(range(6, 8)), list(range(8, 12)))), cen, rad), cen, rad)


@pytest.mark.parametrize("field,delta", [("lmin", +1), ("lmax", -1), ("rmin", +1), ("rmax", -1)])
def test_a_shrunk_box_fails(field, delta):
    nodes, recs, ids, info, cen, rad = _two_leaves()
    nodes[0][field][1] = np.nextafter(nodes[0][field][1], np.float32(np.inf * delta))
    with pytest.raises(BvhError, match="box of child"):
        check_bvh(nodes, recs, ids, info, cen, rad)


@pytest.mark.parametrize("field,delta", [("lmin", -1), ("lmax", +1), ("rmin", -1), ("rmax", +1)])
def test_a_grown_box_fails(field, delta):
    nodes, recs, ids, info, cen, rad = _two_leaves()
    nodes[0][field][2] = np.nextafter(nodes[0][field][2], np.float32(np.inf * delta))
    with pytest.raises(BvhError, match="box of child"):
        check_bvh(nodes, recs, ids, info, cen, rad)


def test_a_missing_sphere_fails():
    cen, rad = _world(8)
    nodes, recs, ids, info = assemble(([0, 1, 2, 3], [4, 5, 6]), cen, rad)         # sphere 7 is nowhere
    with pytest.raises(BvhError):
        check_bvh(nodes, recs, ids, info, cen, rad)
    # ... also when the tables have the right length: sphere 7's record is there, no leaf refers to it
    ids8 = np.append(ids, 7).astype(np.uint32)
    recs8 = np.concatenate([recs, [[*cen[7], rad[7] * rad[7]]]]).astype(np.float32)
    info["plan"]["device_bytes"] += 20
    with pytest.raises(BvhError, match="sphere 7 is in no leaf"):
        check_bvh(nodes, recs8, ids8, info, cen, rad)


def test_a_duplicated_sphere_fails():
    cen, rad = _world(8)
    nodes, recs, ids, info = assemble(([0, 1, 2, 3], [3, 4, 5, 6]), cen, rad)      # 3 twice, 7 missing: lengths are right
    with pytest.raises(BvhError, match="sphere 7 is in no leaf|sphere 3 is tested 2 times"):
        check_bvh(nodes, recs, ids, info, cen, rad)
    # the same leaf referred to twice
    nodes, recs, ids, info = assemble(([0, 1, 2, 3], [4, 5, 6, 7]), cen, rad)
    nodes[0]["right"], nodes[0]["rmin"], nodes[0]["rmax"] = nodes[0]["left"], nodes[0]["lmin"], nodes[0]["lmax"]
    with pytest.raises(BvhError, match="is in no leaf|tested 2 times"):
        check_bvh(nodes, recs, ids, info, cen, rad)


def test_a_five_sphere_leaf_fails():
    cen, rad = _world(9)
    with pytest.raises(BvhError, match="a leaf of 5 spheres"):
        check_bvh(*assemble(([0, 1, 2, 3, 4], [5, 6, 7, 8]), cen, rad), cen, rad)


def _chain(depth):
    """`depth` inner nodes in a chain, one sphere hanging off every one: the deepest leaves lie at `depth`."""
    t = ([depth - 1], [depth])
    for i in range(depth - 2, -1, -1):
        t = ([i], t)
    return t


def test_a_depth_32_chain_passes_and_a_depth_33_chain_fails():
    cen, rad = _world(34, seed=3)
    count = check_bvh(*assemble(_chain(32), cen[:33], rad[:33]), cen[:33], rad[:33])
    assert count["max_depth"] == 32 and count["n_nodes"] == 32
    with pytest.raises(BvhError, match="depth 3[23]"):
        check_bvh(*assemble(_chain(33), cen, rad), cen, rad)


def test_wrong_records_bounds_and_counts_fail():
    nodes, recs, ids, info, cen, rad = _two_leaves()
    bad = recs.copy()
    bad[2, 3] = np.nextafter(bad[2, 3], np.float32(1))
    with pytest.raises(BvhError, match="record"):
        check_bvh(nodes, bad, ids, info, cen, rad)
    for key, value, what in (("radius", info["radius"] * 0.5, "radius"), ("r_max", 0.01, "r_max")):
        with pytest.raises(BvhError, match=what):
            check_bvh(nodes, recs, ids, {**info, key: value}, cen, rad)
    with pytest.raises(BvhError, match="info.plan.n_leaves"):
        check_bvh(nodes, recs, ids, {**info, "plan": {**info["plan"], "n_leaves": 3}}, cen, rad)


def test_non_finite_and_zero_radius_spheres():
    cen, rad = _world(8, seed=4)
    cen[2, 0] = np.inf
    rad[6] = np.nan
    rad[1] = 0.0
    assert always_list(cen, rad).tolist() == [2, 6]
    check_bvh(*assemble(([0, 1, 3], [4, 5, 7]), cen, rad, always=[2, 6]), cen, rad)
    lo, hi = sphere_boxes(cen, rad)
    assert np.all(lo[2] == -np.inf) and np.all(hi[6] == np.inf)
    assert np.all(lo[1] < cen[1]) and np.all(hi[1] > cen[1])                     # the 2^-20 pad keeps a zero radius inside an open box


def test_the_always_list_has_the_length_the_host_plan_reports():
    """Without a device the host tree is described by mirt_bvh_plan alone; the length of its always-tested list can be compared."""
    import weekend_raytracer_wgpu_amd as m
    from hbm_worlds import c_spheres, rtiow_field
    arr, _, _ = rtiow_field(3000)
    plan = m.bvh_plan(c_spheres(arr)[0])
    assert plan["n_always"] == len(always_list(arr["center"][:, :3], arr["radius"]))
