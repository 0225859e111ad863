"""The HBM BVH walk (nearest_hit_bvh) where its SLACK decides records: the ray sets of tests/bvh_rounding.py through four trees each,
and the scenes of tests/grid_rounding.py -- which so far only the LDS grid builds saw -- as MIRT_SCENE_HBM scenes.

References: the flat scan restated on the CPU (ray_query_ref), the flat scan on the device (MIRT_RAYS_FLAT, flat=True, MIRT_FLAG_NO_GRID),
the LDS default build and the oracle.  For the trees the device really walks, the numpy walk of tests/bvh_walk_ref.py reproduces the
device's records with the kernel's constants and changes at least 16 of them without the growth E of the boxes: the comparisons
below can fail.  Every comparison is exact; a failure names the set, the tree, the kernel and the first ray or the pixel count."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from bvh_check import check_bvh
import bvh_rounding as br
import grid_rounding as gr
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

FLAT, ANY, SORT = m.MIRT_RAYS_FLAT, m.MIRT_RAYS_ANY_HIT, m.MIRT_RAYS_SORT
PT, POOL, NO_GRID = m.MIRT_MODE_PT, m.MIRT_FLAG_KERNEL_POOL, m.MIRT_FLAG_NO_GRID
TREES = ["host", "device", "set_spheres", "refit"]
STRIP = "render_pt_hbm_kernel<false,false,true,true>"
STRIP_FRAME = "render_pt_hbm_frame_kernel<false,false,true,true>"
TF = ("false", "true")
RADIANCE_SPP, RADIANCE_BOUNCES = 2, 4


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lds_ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _rows(a):
    return _bytes(a).reshape(len(a), -1)


def _jittered(arr, seed=61):
    """The world with every centre moved by up to one radius along each axis: where the refitted tree starts from."""
    rng = np.random.default_rng(seed)
    moved = arr.copy()
    moved["center"][:, :3] += (rng.uniform(-1, 1, (len(arr), 3)) * np.abs(arr["radius"])[:, None]).astype(np.float32)
    return moved


def _make_tree(ctx, arr, tree):
    """The world `arr` resident on `ctx` behind the tree `tree`; returns the tree read back, validated by check_bvh."""
    if tree in ("host", "device"):
        ctx.set_scene(rq.scene_of(arr), hbm=True, bvh=tree)
        assert ctx.bvh_info()["built_on_device"] == (tree == "device")
    elif tree == "set_spheres":
        ctx.set_scene(rq.scene_of(rq.set_c()[0]), hbm=True)          # another world, host-built: 2 197 spheres
        ctx.set_spheres(arr)
        assert ctx.bvh_info()["built_on_device"]
    else:
        ctx.set_scene(rq.scene_of(_jittered(arr)), hbm=True)
        ctx.update_spheres(0, arr)
        assert ctx.bvh_refits() == 1
    nodes, recs, ids = ctx.bvh_read()
    info = ctx.bvh_info()
    check_bvh(nodes, recs, ids, info, *rq.world_arrays(arr))
    return nodes, recs, ids, info


def _same_records(got, want, what, rays=None):
    bad = np.nonzero(~rq.same_bits(got, want))[0]
    print(f"{what}: {len(bad)} of {len(got)} records differ")
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(got)} records differ, first ray {bad[0]}" + (f" {rays[bad[0]]}" if rays is not None else "")
                           + f": got {got[bad[0]]}, want {want[bad[0]]}")


def _same_bytes(got, want, what):
    bad = np.nonzero((_rows(got) != _rows(want)).any(1))[0]
    print(f"{what}: {len(bad)} of {len(got)} records differ")
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first ray {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _radiance_pool_name(ctx):
    depth = ctx.bvh_info()["plan"]["max_depth"]
    plan = m.bvh_pool_plan(depth)
    assert plan["slots"] != 0 and plan["stack_entries"] == depth
    return "radiance_rays_pool_kernel<%d,%d,4,false,false>" % (plan["threads"], plan["slots"])


# ---- 1. every set through four trees: ray queries and radiance queries ----

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", list(br.SETS))
def test_ray_sets_through_four_trees(ctx, name, tree):
    arr, o, d = br.ray_set(name)
    _make_tree(ctx, arr, tree)
    what = f"{name}, {tree} tree"
    rays, want = br.rays_of(name), br.reference(name)
    got = ctx.trace_rays(rays)
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,false>", ctx.last_kernel()
    flat = ctx.trace_rays(rays, FLAT)
    assert ctx.last_kernel() == "trace_rays_kernel<false,false,false>", ctx.last_kernel()
    _same_records(flat, want, f"{what}, trace_rays_kernel<false,false,false> against the CPU reference", rays)
    _same_bytes(got, flat, f"{what}, trace_rays_kernel<true,false,false> against MIRT_RAYS_FLAT")
    _same_records(got, want, f"{what}, trace_rays_kernel<true,false,false> against the CPU reference", rays)
    any_hit = ctx.trace_rays(rays, ANY)
    assert ctx.last_kernel() == "trace_rays_kernel<true,true,false>", ctx.last_kernel()
    _same_bytes(any_hit, rq.any_hit_of(want), f"{what}, trace_rays_kernel<true,true,false> against any_hit_of the reference")
    sorted_ = ctx.trace_rays(rays, SORT)
    assert ctx.last_kernel() == "trace_rays_sorted_kernel<true,false,false>", ctx.last_kernel()
    _same_bytes(sorted_, got, f"{what}, trace_rays_sorted_kernel<true,false,false> against the unsorted call")
    # the same rays as radiance queries: the walk from the bounce origins as well
    rr = m.make_radiance_rays(o, d)
    kw = dict(num_bounces=RADIANCE_BOUNCES, seed=5)
    plain = ctx.trace_radiance(rr, RADIANCE_SPP, **kw)
    assert ctx.last_kernel() == "radiance_rays_kernel<false,true>", ctx.last_kernel()
    flat_r = ctx.trace_radiance(rr, RADIANCE_SPP, flat=True, **kw)
    assert ctx.last_kernel() == "radiance_rays_kernel<false,false>", ctx.last_kernel()
    _same_bytes(plain, flat_r, f"{what}, radiance_rays_kernel<false,true> against flat=True")
    pooled = ctx.trace_radiance(rr, RADIANCE_SPP, pool=True, **kw)
    assert ctx.last_kernel() == _radiance_pool_name(ctx), ctx.last_kernel()
    _same_bytes(pooled, plain, f"{what}, {ctx.last_kernel()} against the unpooled call")
    sorted_r = ctx.trace_radiance(rr, RADIANCE_SPP, sort=True, **kw)
    assert ctx.last_kernel() == "radiance_rays_sorted_kernel<false,true>", ctx.last_kernel()
    _same_bytes(sorted_r, plain, f"{what}, radiance_rays_sorted_kernel<false,true> against the unsorted call")
    assert (plain["samples"] == RADIANCE_SPP).all()


# ---- 2. the audit: on the trees the device walks, the comparison can fail ----

@pytest.mark.parametrize("tree", ["host", "device"])
@pytest.mark.parametrize("name", br.AUDITED)
def test_the_devices_trees_need_the_slack(ctx, name, tree):
    arr, o, d = br.ray_set(name)
    read = _make_tree(ctx, arr, tree)
    sub = br.audit_subset(name)
    assert len(sub) <= 1024
    got = ctx.trace_rays(br.rays_of(name)[sub])
    assert ctx.last_kernel() == "trace_rays_kernel<true,false,false>"
    kernel = br.walk_tree(read, name, "kernel", sub)
    _same_records(kernel, got, f"{name}, {tree} tree: the numpy walk with the kernel's constants against the device")
    row = {mu: br.changed(br.walk_tree(read, name, mu, sub), kernel) for mu in ("E = 0", "E / 2^4", "slack = 1", "no 2 r_max")}
    reach = br.reaches(name)[sub]
    print(f"{name}, {tree} tree (depth {read[3]['plan']['max_depth']}): {len(sub)} rays, {int((got['sphere'] != rq.MISS).sum())} hits, "
          f"{int((reach > 0).sum())} phantom winners, records changed: " + ", ".join(f"{mu}: {n}" for mu, n in row.items()))
    assert row["E = 0"] >= br.FLOOR


# ---- 3. the scenes of the LDS grid test as HBM scenes ----

def _bounces(scene):
    return 6 if scene == "far origins" else 4


def _sums(c, p):
    c.accum_reset(p)
    c.accum_add(p)
    return c.accum_read(p)


def _frame_sums(c, p, w, h):
    import torch
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.accum_reset(p)
    c.accum_frame_device(p, out.data_ptr())
    c.synchronize()
    return c.accum_read(p), out.cpu().numpy()


def _pooled_name(ctx, frame=False):
    plan = m.bvh_pool_plan(ctx.bvh_info()["plan"]["max_depth"])
    assert plan["slots"] != 0
    return "render_pt_pool_hbm%s_kernel<%d,%d,4,false,false>" % ("_frame" if frame else "", plan["threads"], plan["slots"])


def _adapt_pool_name(ctx):
    plan = m.adapt_pool_plan(ctx.bvh_info()["plan"]["max_depth"])
    assert plan["slots"] != 0
    return "adapt_pixels_pool_kernel<%d,%d,4,false>" % (plan["threads"], plan["slots"])


# build name -> (flags, spp)
BUILDS = {"strip 3 spp": (0, 3), "strip 8 spp": (0, 8), "pool 24 spp": (POOL, 24)}


@pytest.mark.parametrize("scene", list(gr.SCENES))
def test_grid_rounding_scenes_as_hbm_scenes(ctx, lds_ctx, oracle, scene):
    sd, w, h = gr.SCENES[scene][0]()
    cen, rad = gr.spheres_of(sd)
    bounces = _bounces(scene)
    failures = []

    def compare(got, want, builder, kernel, against):
        n = int((got != want).any(axis=-1).sum())
        print(f"{scene} | {builder} tree | {kernel} | against {against}: {n} of {w * h} pixels differ")
        if n:
            failures.append(f"{scene} | {builder} tree | {kernel} | against {against}: {n} of {w * h} pixels differ")

    def params(name, extra=0):
        flags, spp = BUILDS[name]
        return m.make_params(w, h, spp, mode=PT, num_bounces=bounces, flags=flags | extra)

    # the LDS default build: what tests/test_gpu_grid_rounding.py holds to the oracle
    lds_ctx.set_scene(sd)
    pf = m.make_params(w, h, 4, mode=PT, num_bounces=bounces)
    lds = {name: _sums(lds_ctx, params(name)) for name in BUILDS}
    lds["frame 4 spp"], lds_image = _frame_sums(lds_ctx, pf, w, h)
    oracle_sums = oracle.render_pt_sums(sd, params("strip 3 spp"))
    for builder in ("host", "device"):
        ctx.set_scene(sd, hbm=True, bvh=builder)
        info = ctx.bvh_info()
        assert info["built_on_device"] == (builder == "device")
        check_bvh(*ctx.bvh_read(), info, cen, rad)
        for name in BUILDS:
            got = _sums(ctx, params(name))
            kernel = ctx.last_kernel()
            assert kernel == (_pooled_name(ctx) if name.startswith("pool") else STRIP), (scene, builder, name, kernel)
            flat = _sums(ctx, params(name, NO_GRID))
            assert ctx.last_kernel().startswith("render_pt_hbm_kernel<false,false,false,"), (scene, builder, name, ctx.last_kernel())
            compare(got, flat, builder, kernel, "MIRT_FLAG_NO_GRID")
            compare(got, lds[name], builder, kernel, "the LDS default build")
            if name == "strip 3 spp":
                compare(got, oracle_sums, builder, kernel, "the oracle")
        got, image = _frame_sums(ctx, pf, w, h)
        assert ctx.last_kernel() == STRIP_FRAME, (scene, builder, ctx.last_kernel())
        flat, flat_image = _frame_sums(ctx, m.make_params(w, h, 4, mode=PT, num_bounces=bounces, flags=NO_GRID), w, h)
        assert ctx.last_kernel().startswith("render_pt_hbm_frame_kernel<false,false,false,"), (scene, builder, ctx.last_kernel())
        compare(got, flat, builder, STRIP_FRAME, "MIRT_FLAG_NO_GRID")
        compare(got, lds["frame 4 spp"], builder, STRIP_FRAME, "the LDS default build")
        compare(image, flat_image, builder, STRIP_FRAME + " (image)", "MIRT_FLAG_NO_GRID")
        compare(image, lds_image, builder, STRIP_FRAME + " (image)", "the LDS default build")
        # a feature frame through the tree and through the flat scan
        p2 = m.make_params(w, h, 2, mode=PT)
        feat = ctx.render_features(p2)
        assert ctx.last_kernel() == "feature_frame_kernel<true>", ctx.last_kernel()
        feat_flat = ctx.render_features(p2, flat=True)
        assert ctx.last_kernel() == "feature_frame_kernel<false>", ctx.last_kernel()
        n = int((_bytes(feat).reshape(h, w, -1) != _bytes(feat_flat).reshape(h, w, -1)).any(-1).sum())
        print(f"{scene} | {builder} tree | feature_frame_kernel<true> | against flat=True: {n} of {w * h} pixels differ")
        if n:
            failures.append(f"{scene} | {builder} tree | feature_frame_kernel<true> | against flat=True: {n} of {w * h} pixels differ")
        # one adaptive step, pooled and unpooled
        pa = m.make_params(w, h, 4, mode=PT, num_bounces=bounces, seed=7)
        records = {}
        for pool in (False, True):
            ctx.adapt_reset(pa)
            ctx.adapt_step(pa, m.make_adapt_params(4, 32, 4096, pool=pool))
            want_name = _adapt_pool_name(ctx) if pool else "adapt_pixels_kernel<false,true>"
            assert ctx.last_kernel() == want_name, (scene, builder, ctx.last_kernel(), want_name)
            records[pool] = ctx.adapt_read()
        assert (records[False]["samples"] == 4).all()
        n = int((_rows(records[True]) != _rows(records[False])).any(1).sum())
        print(f"{scene} | {builder} tree | {_adapt_pool_name(ctx)} | against adapt_pixels_kernel<false,true>: {n} of {w * h} pixels differ")
        if n:
            failures.append(f"{scene} | {builder} tree | {_adapt_pool_name(ctx)} | against adapt_pixels_kernel<false,true>: {n} of {w * h} pixels differ")
    assert not failures, "\n".join([f"{len(failures)} comparisons differ:"] + failures)
