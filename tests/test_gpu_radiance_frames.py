"""mirt_ctx_trace_radiance* held to the CPU oracle on whole frames (tests/radiance_frames.py): a query of the renderer's own primary
rays of one sample index, with stream = pixel index, must return the oracle's 1-spp frame at that sample_begin, record by record and
bit by bit -- w * h records per oracle render, which is what lets the judge reach 3 015-ray frames with a ragged last wave, a lens
camera (an origin per lane), trees 22 to 32 levels deep whose traversal stacks fill to the last of path_radiance's 32 entries (with
and without the 144-byte sky blob in front of the stacks), a refitted tree, 72 360 rays in 1 131 blocks, streams up to 0xFFFFFFFF and
the degenerate worlds.  Every case asserts the launch's own name, first that the tree's bytes equal the flat scan's, then that they
equal the oracle's.  One context for the module; what the fixtures are worth is asserted on the CPU alone in
tests/test_radiance_frames_cpu.py.

Measured on an MI355X (what the audit of test_deep_frames prints for the 1 536 rays of sample 0): sp reaches plan.max_depth on all
1 536 rays of every staircase, and one entry fewer changes the first hit of 494 (stair22), 404 (stair25), 205 (stair28) and 69
(stair32) of them; on line32 under the long camera sp reaches 32 on 570 rays, none of which hits (what the deepest push guards lies
below MIN_T there: see tests/test_gpu_deep_trees.py)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE
from bvh_walk_ref import walk
import deep_worlds as dw
import feature_ref as fr
import hbm_worlds
import radiance_frames as rf
import radiance_ref as rr
import ray_query_ref as rq
from test_gpu_deep_trees import BOUNCES, ONCE, STACK_EDGE, WORLDS, _cameras
from test_gpu_deep_trees import _set as _set_deep
from test_gpu_trace_radiance import SUBSET

pytestmark = pytest.mark.gpu

BVH = pytest.mark.parametrize("bvh", ["host", "device"])
W, H = fr.W, fr.H                           # 67 x 45 = 3 015 rays: 47 full waves and one of 7 live lanes
DW, DH = rf.DEEP_W, rf.DEEP_H
PT = m.MIRT_MODE_PT
AUDIT_SAMPLE = 0                            # the sample index whose rays the stack audit walks: sample 0 fills the stacks on every world
assert SUBSET == rf.SUBSET and (DW, DH) == (48, 32) and W * H == 47 * 64 + 7


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _name(hosek, bvh):
    tf = ("false", "true")
    return f"radiance_rays_kernel<{tf[hosek]},{tf[bvh]}>"


def _differ(a, b):
    return np.nonzero((_bytes(a).reshape(-1, 32) != _bytes(b).reshape(-1, 32)).any(1))[0]


def _tree_is_flat(tree, flat, what):
    assert tree.dtype == flat.dtype == RADIANCE_DTYPE and tree.shape == flat.shape
    bad = _differ(tree, flat)
    assert len(bad) == 0, f"{what}: tree != flat on {len(bad)} of {len(tree)} records, first {bad[0]}: tree {tree[bad[0]]}, flat {flat[bad[0]]}"


def _agree(got, want, what):
    bad = _differ(got, want)
    print(f"{what}: {len(got)} records, {len(bad)} differ from the oracle")
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ from the oracle, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _frame(ctx, cam, w, h, samples, what, hosek=False, **kw):
    """query_frame through the tree, after checking that the flat scan on the device returns the same bytes."""
    tree = rf.query_frame(ctx, cam, w, h, samples, hosek=hosek, **kw)
    assert ctx.last_kernel() == _name(hosek, True), ctx.last_kernel()
    flat = rf.query_frame(ctx, cam, w, h, samples, hosek=hosek, flat=True, **kw)
    assert ctx.last_kernel() == _name(hosek, False), ctx.last_kernel()
    _tree_is_flat(tree, flat, what)
    assert (tree["samples"] == len(samples)).all() and not tree["_pad"].any()
    return tree


def _batch(ctx, rays, spp, what, hosek=False, **kw):
    tree = ctx.trace_radiance(rays, spp, hosek=hosek, **kw)
    assert ctx.last_kernel() == _name(hosek, True), ctx.last_kernel()
    flat = ctx.trace_radiance(rays, spp, hosek=hosek, flat=True, **kw)
    assert ctx.last_kernel() == _name(hosek, False), ctx.last_kernel()
    _tree_is_flat(tree, flat, what)
    return tree


def _rendered(ctx, w, h, begin, count, **kw):
    """The render kernel as a second witness: uint64 [w * h, 3], the sums mirt_ctx_accum_add gives samples begin .. begin + count - 1
    (an accumulation starts at sample 0: the sums of the first `begin` samples are taken off those of begin + count)."""
    def upto(n):
        p = m.make_params(w, h, n, mode=PT, **kw)
        ctx.accum_reset(p)
        ctx.accum_add(p)
        assert ctx.accum_samples() == n
        return ctx.accum_read(p).reshape(-1, 3)
    sums = upto(begin + count)
    assert "render_pt_hbm_kernel" in ctx.last_kernel(), ctx.last_kernel()
    return sums - upto(begin) if begin else sums


# ---- a. whole frames on the feature fixture ----

def _set_fixture(ctx, bvh, aperture=0.0, sky=None, arr=None):
    ctx.set_scene(rf.fixture_scene_of(fr.fixture().arr if arr is None else arr, aperture, sky), hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


@BVH
def test_whole_frames_of_the_fixture(ctx, bvh):
    pin, lens = fr.fixture_camera(), fr.fixture_camera(aperture=0.1)
    sd = fr.fixture_scene()
    _set_fixture(ctx, bvh)
    assert ctx.bvh_info()["plan"]["max_depth"] >= 10
    what = f"fixture, {bvh} tree, samples 0 1 2"
    got = _frame(ctx, pin, W, H, (0, 1, 2), what)
    _agree(got, rf.frame_records(sd, W, H, (0, 1, 2), 8), what)
    assert np.array_equal(got["sum"], _rendered(ctx, W, H, 0, 3, num_bounces=8)), f"{what}: against the render kernel's accumulation"
    # a seed with both halves set, from sample 5 on
    what = f"fixture, {bvh} tree, a seed and samples 5 6"
    got = _frame(ctx, pin, W, H, (5, 6), what, seed=rr.SEED)
    _agree(got, rf.frame_records(sd, W, H, (5, 6), 8, seed=rr.SEED), what)
    assert np.array_equal(got["sum"], _rendered(ctx, W, H, 5, 2, num_bounces=8, seed=rr.SEED)), f"{what}: against the render kernel's accumulation"
    # 1 and 300 bounces on one sample
    for nb in (1, 300):
        what = f"fixture, {bvh} tree, {nb} bounces"
        got = _frame(ctx, pin, W, H, (0,), what, num_bounces=nb)
        _agree(got, rf.frame_records(sd, W, H, (0,), nb), what)
        assert np.array_equal(got["sum"], _rendered(ctx, W, H, 0, 1, num_bounces=nb)), f"{what}: against the render kernel's accumulation"
    # the lens camera: an origin per lane
    _set_fixture(ctx, bvh, aperture=0.1)
    what = f"fixture through a lens, {bvh} tree, samples 0 1"
    got = _frame(ctx, lens, W, H, (0, 1), what)
    _agree(got, rf.frame_records(fr.fixture_scene(0.1), W, H, (0, 1), 8), what)
    assert np.array_equal(got["sum"], _rendered(ctx, W, H, 0, 2, num_bounces=8)), f"{what}: against the render kernel's accumulation"
    # the Hosek build with a sky blob
    _set_fixture(ctx, bvh, sky=rr.sky_blob())
    what = f"fixture under the Hosek sky, {bvh} tree, samples 0 1"
    got = _frame(ctx, pin, W, H, (0, 1), what, hosek=True)
    _agree(got, rf.frame_records(rf.fixture_scene_with_sky(), W, H, (0, 1), 8, hosek=True), what)
    assert np.array_equal(got["sum"], _rendered(ctx, W, H, 0, 2, num_bounces=8, flags=m.MIRT_FLAG_SKY_HOSEK)), f"{what}: against the render kernel"


# ---- b. full stacks ----

def _audit(ctx, name, view, cam, depth):
    """The numpy walk (bound kMaxT) on the very rays of sample AUDIT_SAMPLE over the tree read back: no push dropped, sp reaches
    plan.max_depth on >= 16 rays, and on the staircases a stack one entry shorter changes the first-hit sphere of >= 16 of them."""
    arr = dw.ray_set(name)[0]
    rays = rf.frame_rays(cam, DW, DH, AUDIT_SAMPLE)
    o, d = rays["origin"].copy(), rays["direction"].copy()
    hits = ctx.trace_rays(rq.rays_of(o, d))
    rad = rq.world_arrays(arr)[1]
    tree, info = ctx.bvh_read(), ctx.bvh_info()
    got, high, dropped = walk(*tree, info, o, d, 1000.0, depth, rad)
    short, _, _ = walk(*tree, info, o, d, 1000.0, depth - 1, rad)
    full = high == depth
    changed = int(((short["sphere"] != got["sphere"]) & full).sum())
    print(f"{name} {view}, sample {AUDIT_SAMPLE}: sp reaches {int(high.max())} of {depth} on {int(full.sum())} of {len(o)} rays, "
          f"{int((hits['sphere'] != rq.MISS).sum())} of them hit; {depth - 1} entries change the first hit of {changed}")
    assert rq.same_bits(got, hits).all() and dropped.sum() == 0 and full.sum() >= 16
    if name in dw.STAIRS:
        assert changed >= 16
    else:
        assert depth == 32 == m.MIRT_BVH_MAX_DEPTH


@pytest.mark.parametrize("name", WORLDS)
def test_deep_frames(ctx, name):
    """Every deep world under every view tests/test_gpu_deep_trees.py renders, by the builder it is made for."""
    views = _cameras(name)
    assert list(views) == list(rf.deep_cameras(name))
    for view, cam in views.items():
        depth = _set_deep(ctx, name, cam)
        what = f"{name} {view}, depth {depth}"
        got = _frame(ctx, cam, DW, DH, (0, 1), what, num_bounces=BOUNCES)
        _agree(got, rf.frame_records(rf.deep_scene(name, cam), DW, DH, (0, 1), BOUNCES), what)
        if (name, view) in STACK_EDGE:
            _audit(ctx, name, view, cam, depth)


@pytest.mark.parametrize("name", ONCE)
def test_deep_frames_with_the_sky_blob_in_front_of_the_stacks(ctx, name):
    cam = list(_cameras(name).values())[-1]                        # the view that fills the stacks
    depth = _set_deep(ctx, name, cam, rr.sky_blob())
    what = f"{name} under the Hosek sky, depth {depth}"
    got = _frame(ctx, cam, DW, DH, (0, 1), what, hosek=True, num_bounces=BOUNCES)
    _agree(got, rf.frame_records(rf.deep_scene(name, cam, rr.sky_blob()), DW, DH, (0, 1), BOUNCES, hosek=True), what)
    plain = rf.query_frame(ctx, cam, DW, DH, (0, 1), num_bounces=BOUNCES)                         # the same scene without the flag
    _agree(plain, rf.frame_records(rf.deep_scene(name, cam), DW, DH, (0, 1), BOUNCES), what + ", queried without the flag")
    assert len(_differ(plain, got)) > 0


def _device_query(ctx, torch, rays, stream, offset=0, preset=0x5A, **kw):
    """trace_radiance_device between torch buffers (4-byte aligned at `offset`) on a caller stream -> the records; the bytes in front
    of the first record and a canary record (and more) behind the last must stay as they were."""
    n = len(rays)
    buf = np.zeros(32 * n + 16, np.uint8)
    buf[offset:offset + 32 * n] = _bytes(rays)
    with torch.cuda.stream(stream):
        d_rays = torch.from_numpy(buf).to("cuda:0", non_blocking=False)
        d_out = torch.full((32 * n + 32 + 16,), preset, dtype=torch.uint8, device="cuda:0")
        ctx.trace_radiance_device(d_rays.data_ptr() + offset, n, d_out.data_ptr() + offset, stream=stream.cuda_stream, **kw)
        out = d_out.cpu().numpy()                                   # ordered after the query on the same stream
    assert (out[:offset] == preset).all() and (out[offset + 32 * n:] == preset).all(), "bytes around the records were written"
    return out[offset:offset + 32 * n].copy().view(RADIANCE_DTYPE)


def test_line32_from_device_memory_on_a_caller_stream(ctx):
    import torch
    cam = _cameras("line32")["long"]
    assert _set_deep(ctx, "line32", cam) == 32
    stream = torch.cuda.Stream(device="cuda:0")
    got = _device_query(ctx, torch, rf.frame_rays(cam, DW, DH, 0), stream, spp=1, num_bounces=BOUNCES)
    assert ctx.last_kernel() == _name(False, True)
    _agree(got, rf.frame_records(rf.deep_scene("line32", cam), DW, DH, (0,), BOUNCES), "line32 long, the device form")


# ---- c. after a refit ----

@BVH
def test_the_frame_of_a_refitted_tree(ctx, bvh):
    import torch
    moved = rf.moved_fixture_world()
    cam = fr.fixture_camera()
    _set_fixture(ctx, bvh)
    before = ctx.bvh_info()
    assert ctx.bvh_refits() == 0
    old = rf.query_frame(ctx, cam, W, H, (0, 1))
    d_moved = torch.from_numpy(_bytes(moved).copy()).to("cuda:0")
    ctx.update_spheres_device(0, len(moved), d_moved.data_ptr())
    info = ctx.bvh_info()
    assert ctx.bvh_refits() == 1 and info["plan"] == before["plan"] and info["root"] == before["root"]       # refitted, not rebuilt
    assert info["built_on_device"] == before["built_on_device"] == (bvh == "device")
    what = f"the moved fixture, refitted {bvh} tree"
    got = _frame(ctx, cam, W, H, (0, 1), what)
    _agree(got, rf.frame_records(rf.fixture_scene_of(moved), W, H, (0, 1), 8), what)
    assert len(_differ(got, old)) > W * H // 10
    _set_fixture(ctx, bvh, arr=moved)
    assert ctx.bvh_refits() == 0
    fresh = rf.query_frame(ctx, cam, W, H, (0, 1))
    assert ctx.last_kernel() == _name(False, True)
    assert np.array_equal(_bytes(fresh), _bytes(got)), f"{what}: against a fresh scene of the moved world"


# ---- d. placement at scale ----

TILES = 24


def test_72360_rays_in_1131_blocks(ctx):
    import torch
    cam = fr.fixture_camera()
    _set_fixture(ctx, "device")
    one = rf.frame_rays(cam, W, H, 0)
    want = rf.frame_records(fr.fixture_scene(), W, H, (0,), 8)
    rays = np.tile(one, TILES)
    n = len(rays)
    assert n == 72360 and (n + 63) // 64 == 1131
    lib = m.lib()
    outs = {}
    for flat in (False, True):
        out = np.zeros(n + 1, RADIANCE_DTYPE)
        _bytes(out)[:] = 0xA5                                       # the canary: record n must stay as it is
        p = _abi.MirtRadianceParams(1, 0, 8, _abi.MIRT_RADIANCE_FLAT if flat else 0, 0)
        assert lib.mirt_ctx_trace_radiance(ctx._h, C.c_void_p(rays.ctypes.data), n, C.byref(p), C.c_void_p(out.ctypes.data)) == 0, lib.mirt_last_error()
        assert ctx.last_kernel() == _name(False, not flat)
        assert (_bytes(out[n:]) == 0xA5).all(), "the record behind the last was written"
        outs[flat] = out[:n]
    _tree_is_flat(outs[False], outs[True], "72 360 rays")
    tiles = _bytes(outs[False]).reshape(TILES, -1)
    assert [k for k in range(TILES) if not np.array_equal(tiles[k], tiles[0])] == [], "a tile's bytes differ from the first tile's"
    _agree(outs[False][:W * H], want, "the first of 24 tiles")
    perm = np.random.default_rng(7).permutation(n)
    shuffled = ctx.trace_radiance(rays[perm], 1)
    assert np.array_equal(_bytes(shuffled), _bytes(outs[False][perm])), "a permutation of the batch"
    stream = torch.cuda.Stream(device="cuda:0")
    got = _device_query(ctx, torch, rays, stream, offset=4, spp=1)
    assert ctx.last_kernel() == _name(False, True)
    assert np.array_equal(_bytes(got), _bytes(outs[False])), "the device form at a 4-byte offset"


# ---- e. high streams ----

@BVH
def test_streams_up_to_0xffffffff_beside_streams_0_to_7(ctx, bvh):
    world, mats, tex = rr.world()
    ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), world, mats, tex), hbm=True, bvh=bvh)
    high, low = rf.high_stream_rays(SUBSET), rr.rays_and_streams(SUBSET)
    rays = np.stack([high, low], 1).reshape(-1)                     # alternating: both waves of the batch mix high and low streams
    want = np.stack([np.concatenate([rf.high_stream_records(i) for i in SUBSET]), rr.oracle_records(SUBSET)], 1).reshape(-1)
    assert len(rays) == 128 and rays["stream"][0] == 0xFFFFFFF8 and rays["stream"][1] == 0 and rays["stream"][14] == 0xFFFFFFFF
    what = f"streams 0xFFFFFFF8 .. 0xFFFFFFFF beside 0 .. 7, {bvh} tree"
    _agree(_batch(ctx, rays, 4, what), want, what)
    what = f"high streams alone, sample_begin 5 and a seed, {bvh} tree"
    got = _batch(ctx, high, 4, what, sample_begin=5, seed=rr.SEED)
    _agree(got, np.concatenate([rf.high_stream_records(i, sample_begin=5, seed=rr.SEED) for i in SUBSET]), what)


# ---- f. degenerate worlds ----

@BVH
@pytest.mark.parametrize("world", list(rf.degenerate_worlds()))
def test_degenerate_worlds(ctx, bvh, world):
    arr = rf.degenerate_worlds()[world]
    cam = rf.degenerate_camera()
    ctx.set_scene(rf.degenerate_scene(arr), hbm=True, bvh=bvh)
    info = ctx.bvh_info()
    if len(arr) == 1:
        assert info["root"] & m.BVH_LEAF
    what = f"{world}, {bvh} tree"
    got = _frame(ctx, cam, rf.SMALL_W, rf.SMALL_H, (0,), what)
    _agree(got, rf.frame_records(rf.degenerate_scene(arr), rf.SMALL_W, rf.SMALL_H, (0,), 8), what)
    assert got["sum"].any(1).all()


# ---- g. a node's member ----

def test_a_nodes_member_answers_as_the_plain_context(ctx):
    cam = fr.fixture_camera()
    _set_fixture(ctx, "host")
    rays = rf.frame_rays(cam, W, H, 0)
    want = ctx.trace_radiance(rays, 1)
    _agree(want, rf.frame_records(fr.fixture_scene(), W, H, (0,), 8), "the plain context")
    node = m.Node([0] * 2)
    try:
        node.set_scene(fr.fixture_scene(), hbm=True)
        member = node.context(1)
        got = member.trace_radiance(rays, 1)
        assert member.last_kernel() == _name(False, True)
        assert np.array_equal(_bytes(got), _bytes(want))
    finally:
        node.close()
