"""MIRT_ADAPT_POOL on the device: an adaptive step whose render stage runs the pooled schedule (adapt_pixels_pool_kernel) must leave
the bytes of the step without the flag -- the list, the count, the 64-bit sample counter and all 64 bytes of every record -- and those
are the bytes of the integer replay of tests/adaptive_ref.py.  Every case asserts the kernel's name first, built from
mirt_adapt_pool_plan of the resident tree's depth, so each fails where the flag is refused.  The shapes are the smallest at which this
kernel can go wrong: ragged units, an empty list, more items than slots (the queues wrap), mixed parities of the sample index inside a
unit, lists of 1 to 65 entries, waves that run several units, a band and a tile partition, every geometry the plan can give."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
import adaptive_ref as ar
import deep_worlds as dw
import hbm_worlds
import radiance_frames as rf
import radiance_ref as rr

pytestmark = pytest.mark.gpu

W, H = ar.W, ar.H
NO_GRID, HOSEK = m.MIRT_FLAG_NO_GRID, m.MIRT_FLAG_SKY_HOSEK
POOL = m.MIRT_ADAPT_POOL
ADAPT = (ar.MIN_SAMPLES, ar.MAX_SAMPLES, ar.TOLERANCE)
TF = ("false", "true")


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _pool_name(ctx, hosek=False, geometry=None):
    """The pooled kernel's name for the resident tree, from mirt_adapt_pool_plan; geometry: the (slots, waves per CU) it must have."""
    depth = ctx.bvh_info()["plan"]["max_depth"]
    plan = m.adapt_pool_plan(depth, hosek)
    assert plan["slots"] != 0 and plan["stack_entries"] == depth
    if geometry is not None:
        assert (plan["slots"], plan["waves_per_cu"]) == geometry, (plan, geometry)
    return "adapt_pixels_pool_kernel<%d,%d,4,%s>" % (plan["threads"], plan["slots"], TF[hosek])


def _plain_name(hosek=False, bvh=True):
    return f"adapt_pixels_kernel<{TF[hosek]},{TF[bvh]}>"


def _same_records(got, want, what):
    assert got.dtype == want.dtype == ADAPT_PIXEL_DTYPE and got.shape == want.shape, what
    bad = np.nonzero((_bytes(got) != _bytes(want)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _steps(ctx, p, adapt, n_steps, name, start=None, stream=None):
    """Reset (and write `start`), then n_steps steps -> per step {"list", "records", "active", "total"}; the kernel's name after every step."""
    ctx.adapt_reset(p)
    if start is not None:
        ctx.adapt_write(start)
    out = []
    for k in range(n_steps):
        ctx.adapt_step(p, adapt, stream=stream)
        assert ctx.last_kernel() == name, (k, ctx.last_kernel(), name)
        st = ctx.adapt_stats()
        assert st["steps"] == k + 1
        out.append({"list": ctx.adapt_list(), "records": ctx.adapt_read(), "active": st["active"], "total": st["total_samples"]})
    return out


def _equal_steps(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        at = f"{what}, step {k + 1}"
        assert g["list"].dtype == np.uint32 and np.array_equal(g["list"], w["list"]), f"{at}: the list differs ({len(g['list'])} entries, want {len(w['list'])})"
        _same_records(g["records"], w["records"], at)
        assert g["total"] == w["total"] and g.get("active", len(w["list"])) == len(w["list"]), (at, g["total"], w["total"])


def _pooled(ctx, p, case, n_steps, want, what, hosek=False, geometry=None, plain=False, start=None, name=None):
    """The pooled loop against the replay `want`; plain=True: and against the same loop without the flag on a second reset."""
    name = name or _pool_name(ctx, hosek, geometry)
    got = _steps(ctx, p, m.make_adapt_params(*case, pool=True), n_steps, name, start)
    print(f"{what}: {name}, lists {[len(g['list']) for g in got]}")
    if want is not None:
        _equal_steps(got, want, what + ", against the replay")
    if plain:
        bvh = not (p.flags & NO_GRID)
        other = _steps(ctx, p, m.make_adapt_params(*case), n_steps, _plain_name(hosek, bvh), start)
        _equal_steps(got, other, what + ", against the step without the flag")
    return got


# ---- 1. the whole loop ----

@pytest.mark.parametrize("bvh", ["host", "device"])
def test_the_whole_loop(ctx, bvh):
    steps = ar.reference_loop()
    lens = [len(s["list"]) for s in steps]
    assert lens == [1536, 731, 599, 486, 401, 333, 273, 243, 0] and [n % 16 for n in lens[1:-1]] == [11, 7, 6, 1, 13, 1, 3]
    ctx.set_scene(ar.scene(), hbm=True, bvh=bvh)
    _pooled(ctx, ar.params(), ADAPT, ar.N_STEPS, steps, f"the whole loop, {bvh} tree", geometry=(112, 16), plain=True)


# ---- 2. more items than slots ----

@pytest.mark.parametrize("hosek", [False, True], ids=["no sky", "hosek"])
def test_refill(ctx, hosek):
    """spp 12: 192 items per unit > 112 slots, so the queues wrap and slots are reused."""
    sd = ar.scene(rr.sky_blob() if hosek else None)
    p = ar.params(spp=12, flags=HOSEK if hosek else 0)
    frames = ar.sample_frames(sd, p, 36, "field300")
    case = (12, 36, 4096)
    steps = ar.replay(frames, 12, *case, 4)
    lens = [len(s["list"]) for s in steps]
    if not hosek:
        assert lens == [1536, 707, 455, 0]
    else:
        assert not np.array_equal(frames, ar.sample_frames(ar.scene(), ar.params(spp=12), 36, "field300"))
        assert lens[0] == 1536 and 0 < lens[2] < lens[1] < 1536 and lens[1] % 16 != 0 and lens[3] == 0
    ctx.set_scene(sd, hbm=True)
    assert 16 * 12 > m.adapt_pool_plan(ctx.bvh_info()["plan"]["max_depth"], hosek)["slots"] == 112
    _pooled(ctx, p, case, 4, steps, f"refill, hosek {hosek}", hosek=hosek, geometry=(112, 16), plain=True)


# ---- 3. the parity of n ----

def test_the_even_half_follows_n_plus_s(ctx):
    frames = ar.sample_frames(ar.scene(), ar.params(), ar.MAX_SAMPLES + ar.SPP, "field300")
    npix = frames.shape[1]
    n0 = (7 * np.arange(npix)) % 5
    start = np.zeros(npix, ADAPT_PIXEL_DTYPE)
    for n in range(1, 5):
        sel = n0 == n
        start["sum"][sel] = frames[:n, sel].sum(axis=0, dtype=np.uint64)
        start["even"][sel] = frames[0:n:2, sel].sum(axis=0, dtype=np.uint64)
    start["samples"] = n0
    case = (4, 32, 4096)
    steps = ar.replay(frames, 4, *case, 4, start=start)
    assert [len(s["list"]) for s in steps] == [1380, 997, 848, 691]
    first = steps[0]["list"]
    for u in range(0, len(first) - 15, 16):                  # both parities inside every full unit of the first step
        assert len(set((n0[first[u:u + 16]] & 1).tolist())) == 2, u
    ctx.set_scene(ar.scene(), hbm=True)
    _pooled(ctx, ar.params(), case, 4, steps, "records that start at n0 = 7 i mod 5", plain=True, start=start)


# ---- 4. small counts ----

@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 65])
def test_small_counts(ctx, k):
    frames = ar.sample_frames(ar.scene(), ar.params(), 8, "field300")
    npix = W * H
    places = np.sort(np.random.default_rng(100 + k).choice(npix, k, replace=False))
    assert k == 1 or ((np.diff(places) > 1).any() and len(set((places // W).tolist())) > 1)      # scattered, across rows
    start = np.zeros(npix, ADAPT_PIXEL_DTYPE)
    start["sum"] = (0x0123456789ABCDEF + 3 * np.arange(npix, dtype=np.uint64))[:, None] + np.arange(3, dtype=np.uint64)
    start["even"] = (0x00FEDCBA98765432 + 5 * np.arange(npix, dtype=np.uint64))[:, None] + np.arange(3, dtype=np.uint64)
    start["samples"] = 8
    start[places] = np.zeros(k, ADAPT_PIXEL_DTYPE)
    case = (8, 8, 0)
    want = ar.replay(frames, 8, *case, 1, start=start)
    assert np.array_equal(want[0]["list"], places)
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params(spp=8)
    got = _pooled(ctx, p, case, 1, want, f"{k} listed records", plain=True, start=start)[0]["records"]
    assert np.array_equal(got["sum"][places], frames[0:8, places].sum(axis=0, dtype=np.uint64))
    assert np.array_equal(got["even"][places], frames[0:8:2, places].sum(axis=0, dtype=np.uint64)) and (got["samples"][places] == 8).all()
    rest = np.ones(npix, bool)
    rest[places] = False
    _same_records(got[rest], start[rest], f"{k} listed records: the others")


# ---- 5. several units per wave ----

def test_waves_that_stride_over_several_units(monkeypatch):
    monkeypatch.setenv("MIRT_ADAPT_POOL_BLOCKS", "1")                  # read when a context is created
    steps = ar.reference_loop()[:3]
    assert [-(-len(s["list"]) // 16) for s in steps[:2]] == [96, 46] and len(steps[1]["list"]) % 16 != 0      # 96 and 46 units on 4 waves
    with m.Context(0) as own:
        own.set_scene(ar.scene(), hbm=True)
        _pooled(own, ar.params(), ADAPT, 3, steps, "one block of four waves", geometry=(112, 16), plain=True)


# ---- 6. a band and a tile partition ----

@pytest.mark.parametrize("rows", [dict(row_begin=8, row_end=24), dict(row_begin=8, row_end=24, tile_rows=4, n_parts=2, part=1)],
                         ids=["band", "tile partition"])
def test_a_band_keeps_the_absolute_pixels_streams(ctx, rows):
    p = ar.params(**rows)
    n_rows = m.params_out_rows(p)
    assert n_rows == (16 if "tile_rows" not in rows else 8)
    frames = ar.sample_frames(ar.scene(), p, 3 * ar.SPP, "field300")
    whole = ar.sample_frames(ar.scene(), ar.params(), 3 * ar.SPP, "field300").reshape(-1, H, W, 3)
    assert not np.array_equal(frames, whole[:, :n_rows].reshape(len(whole), -1, 3))      # not the rows a band-relative index would take
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert 0 < len(steps[2]["list"]) < len(steps[1]["list"]) < n_rows * W
    ctx.set_scene(ar.scene(), hbm=True)
    _pooled(ctx, p, ADAPT, 3, steps, f"rows {rows}", plain=True)


# ---- 7. deep trees ----

def _deepest_small_world():
    """The world and view tests/test_gpu_adaptive.py's full-stack test picks: the smallest of tests/deep_worlds.py whose tree is 32 deep."""
    deep = [n for n in list(dw.LINES) + list(dw.STAIRS) if (dw.DEVICE_DEPTH[n] if n in dw.STAIRS else dw.HOST_DEPTH[n]) == 32]
    name = min(deep, key=lambda n: len(dw.ray_set(n)[0]))
    return name, list(rf.deep_cameras(name))[-1]


def _deep(ctx, name, view, depth, geometry):
    cam = rf.deep_cameras(name)[view]
    sd = rf.deep_scene(name, cam)
    ctx.set_scene(sd, hbm=True, bvh="device" if name in dw.STAIRS else "host")
    assert ctx.bvh_info()["plan"]["max_depth"] == depth
    w, h = rf.DEEP_W, rf.DEEP_H
    p = ar.params(w=w, h=h, bounces=6)
    frames = ar.sample_frames(sd, p, 8, name + view)
    steps = ar.replay(frames, ar.SPP, 4, 8, 256, 2)
    assert len(steps[0]["list"]) == w * h and 0 < len(steps[1]["list"]) < w * h
    _pooled(ctx, p, (4, 8, 256), 2, steps, f"{name} ({view}), depth {depth}", geometry=geometry, plain=True)
    assert ctx.last_kernel() == _plain_name() and f",{geometry[0]},4," in _pool_name(ctx)


def test_full_stacks_on_a_tree_32_deep(ctx):
    name, view = _deepest_small_world()
    _deep(ctx, name, view, 32, (80, 12))


def test_a_tree_28_deep_takes_96_slots(ctx):
    assert dw.DEVICE_DEPTH["stair28"] == 28
    _deep(ctx, "stair28", "far", 28, (96, 12))


# ---- 8. forced geometries ----

@pytest.mark.parametrize("slots", [80, 64])
def test_forced_geometries_on_a_shallow_tree(monkeypatch, slots):
    monkeypatch.setenv("MIRT_HBM_POOL_SLOTS", str(slots))              # read when a context is created
    with m.Context(0) as own:
        own.set_scene(ar.scene(), hbm=True)
        assert m.adapt_pool_plan(own.bvh_info()["plan"]["max_depth"])["slots"] == 112      # the plan alone would take 112 slots
        _pooled(own, ar.params(), ADAPT, 2, ar.reference_loop()[:2], f"{slots} slots forced", plain=True,
                name=f"adapt_pixels_pool_kernel<256,{slots},4,false>")


# ---- 9. where the pool stops ----

def test_not_pooled(ctx):
    ctx.set_scene(ar.scene(), hbm=True)
    steps = ar.reference_loop()[:2]
    _pooled(ctx, ar.params(flags=NO_GRID), ADAPT, 2, steps, "MIRT_FLAG_NO_GRID | pool", plain=True, name=_plain_name(False, False))
    p = ar.params(bounces=256)
    got = _pooled(ctx, p, ADAPT, 1, None, "num_bounces 256 | pool", plain=True, name=_plain_name())
    assert len(got[0]["list"]) == W * H


@pytest.mark.parametrize("bounces", [0, 1, 255])
def test_bounce_limits_that_are_pooled(ctx, bounces):
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params(bounces=bounces)
    steps = ar.replay(ar.sample_frames(ar.scene(), p, ar.SPP, "field300"), ar.SPP, *ADAPT, 1)
    got = _pooled(ctx, p, ADAPT, 1, steps, f"num_bounces {bounces}", geometry=(112, 16), plain=True)
    assert bool(got[0]["records"]["sum"].any()) == (bounces != 0)      # no bounce: no path reaches the sky, every sample is black


# ---- 10. refusals with the flag set leave no trace ----

def test_refusals_leave_no_trace(ctx):
    lib = m.lib()
    ctx.set_scene(ar.scene(), hbm=True)
    p, adapt = ar.params(), m.make_adapt_params(*ADAPT, pool=True)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    accum_before, stats_before = ctx.accum_read(p).copy(), ctx.stats()
    ctx.adapt_reset(p)
    ctx.adapt_step(p, adapt)
    ctx.adapt_step(p, adapt)
    kernel_before = ctx.last_kernel()
    assert kernel_before == _pool_name(ctx, geometry=(112, 16))
    before, list_before, st_before = ctx.adapt_read(), ctx.adapt_list(), ctx.adapt_stats()
    _same_records(before, ar.reference_loop()[1]["records"], "two pooled steps")

    def refused(params, ad, code, what):
        rc = lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(params), C.byref(ad), None)
        assert rc == code, f"{what}: {_abi.STATUS.get(rc, rc)} ({lib.mirt_last_error().decode()})"
        _same_records(ctx.adapt_read(), before, what)
        st = ctx.adapt_stats()
        assert np.array_equal(ctx.adapt_list(), list_before) and (st["steps"], st["total_samples"], st["active"]) == \
            (st_before["steps"], st_before["total_samples"], st_before["active"]), what
        assert ctx.last_kernel() == kernel_before

    for flags in (1, 3, 4, POOL | 4):
        bad = m.make_adapt_params(*ADAPT)
        bad.flags = flags
        refused(p, bad, _abi.MIRT_ERR_BAD_MODE, f"adapt->flags {flags:#x}")
    refused(ar.params(spp=3), adapt, _abi.MIRT_ERR_SPP_RANGE, "odd spp")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PT, seed=ar.SEED, frame_spp=2), adapt, _abi.MIRT_ERR_FRAME_SPP, "frame_spp != 0")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_WORK")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_GRID")
    refused(ar.params(w=W + 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another width")
    refused(ar.params(row_begin=0, row_end=H - 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another row count")
    refused(ar.params(spp=0), adapt, _abi.MIRT_ERR_SPP_ZERO, "spp == 0")
    refused(ar.params(flags=HOSEK), adapt, _abi.MIRT_ERR_SKY, "MIRT_FLAG_SKY_HOSEK without a blob")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PARITY), adapt, _abi.MIRT_ERR_BAD_MODE, "parity mode")
    refused(p, m.make_adapt_params(4, _abi.MIRT_MAX_SPP_PER_CALL + 1, 4096, pool=True), _abi.MIRT_ERR_SPP_RANGE, "max_samples above the per-call limit")
    assert lib.mirt_ctx_adapt_step_device(ctx._h, None, C.byref(adapt), None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(p), None, None) == _abi.MIRT_ERR_NULL_POINTER
    _same_records(ctx.adapt_read(), before, "after the null pointers")
    # pooled steps touched neither the accumulation nor MirtStats
    assert np.array_equal(ctx.accum_read(p), accum_before) and ctx.accum_samples() == 4
    stats_after = ctx.stats()
    assert stats_after["launches"] == 0 and stats_after["samples"] == stats_before["samples"] and stats_after["kernel_ms"] == stats_before["kernel_ms"]
    # no MIRT_SCENE_HBM scene: an LDS scene refuses the step, and a fresh context too
    ctx.set_scene(ar.scene())
    refused(p, adapt, _abi.MIRT_ERR_NO_SCENE, "an LDS scene")
    with m.Context(0) as fresh:
        assert lib.mirt_ctx_adapt_step_device(fresh._h, C.byref(p), C.byref(adapt), None) == _abi.MIRT_ERR_NO_SCENE
        assert fresh.adapt_stats() == {"pixels": 0, "total_samples": 0, "active": 0, "steps": 0, "kernel_ms": 0.0}


# ---- 11. other call paths ----

def _moved_field(seed=5):
    """The fixture's spheres, every centre moved a little: same count, same materials (a refit keeps the tree's shape)."""
    arr, mats, tex = ar._field()
    moved = arr.copy()
    moved["center"][:, :3] += np.random.default_rng(seed).uniform(-0.04, 0.04, (len(arr), 3)).astype(np.float32)
    return moved, mats, tex


def test_the_device_form_and_worlds_changed_on_the_device(ctx):
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx.set_scene(ar.scene(), hbm=True, bvh="device")
    p, adapt = ar.params(), m.make_adapt_params(*ADAPT, pool=True)
    steps = ar.reference_loop()[:3]
    torch.cuda.synchronize()
    got = _steps(ctx, p, adapt, 3, _pool_name(ctx, geometry=(112, 16)), stream=stream.cuda_stream)
    _equal_steps(got, steps, "the device form on a caller's stream")
    assert ctx.adapt_stats()["kernel_ms"] > 0.0
    # a refit: same tree, same depth, moved spheres
    moved, mats, tex = _moved_field()
    before = ctx.bvh_info()
    d_moved = torch.from_numpy(_bytes(moved).copy()).to("cuda:0")
    ctx.update_spheres_device(0, len(moved), d_moved.data_ptr())
    assert ctx.bvh_refits() == 1 and ctx.bvh_info()["plan"] == before["plan"]
    sd = hbm_worlds.scene_from_arrays(ar.camera(), moved, mats, tex)
    frames = ar.sample_frames(sd, p, 2 * ar.SPP, "field300 moved")
    assert not np.array_equal(frames, ar.sample_frames(ar.scene(), p, 2 * ar.SPP, "field300"))
    _pooled(ctx, p, ADAPT, 2, ar.replay(frames, ar.SPP, *ADAPT, 2), "after update_spheres_device", geometry=(112, 16), plain=True)
    # a world replaced from device memory: a depth-8 tree, then a deeper one -- the geometry and the name follow the new depth
    name = "stair22"
    dcam = rf.deep_cameras(name)["far"]
    arr = dw.ray_set(name)[0]
    fmats, ftex = hbm_worlds.field_materials()
    copies = hbm_worlds.sphere_array(np.tile([[0.0, 1.0, 0.0]], (1000, 1)), np.full(1000, 1.0), np.zeros(1000))
    ctx.set_scene(hbm_worlds.scene_from_arrays(dcam, copies, fmats, ftex), hbm=True)
    assert ctx.bvh_info()["plan"]["max_depth"] == 8
    q = ar.params(w=rf.DEEP_W, h=rf.DEEP_H, bounces=6)
    _steps(ctx, q, m.make_adapt_params(4, 8, 256, pool=True), 1, _pool_name(ctx, geometry=(112, 16)))
    d_arr = torch.from_numpy(_bytes(arr).copy()).to("cuda:0")
    ctx.set_spheres_device(len(arr), d_arr.data_ptr())
    assert ctx.bvh_info()["plan"]["max_depth"] == dw.DEVICE_DEPTH[name] == 22
    frames = ar.sample_frames(rf.deep_scene(name, dcam), q, 8, name + "far")
    _pooled(ctx, q, (4, 8, 256), 2, ar.replay(frames, ar.SPP, 4, 8, 256, 2), "after set_spheres_device to a tree of depth 22", plain=True,
            name="adapt_pixels_pool_kernel<256,64,4,false>", geometry=(64, 16))
    assert _pool_name(ctx, geometry=(64, 16)) == "adapt_pixels_pool_kernel<256,64,4,false>"


def test_raytracer_render_adaptive_pooled():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(W, H), sampling=m.SamplingParams(max_samples_per_pixel=32, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        img, counts = rt.render_adaptive(4096, 32, seed=3, pool=True)
        assert rt._ctx.last_kernel() == _pool_name(rt._ctx), rt._ctx.last_kernel()
        total = rt._ctx.adapt_stats()["total_samples"]
        img0, counts0 = rt.render_adaptive(4096, 32, seed=3, pool=False)
        assert rt._ctx.last_kernel() == _plain_name()
        assert np.array_equal(img, img0) and np.array_equal(counts, counts0) and total == int(counts.sum()) == rt._ctx.adapt_stats()["total_samples"]
        assert len(np.unique(counts)) > 2
    finally:
        rt.close()
