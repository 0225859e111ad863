"""mirt_ctx_adapt_* on the device, held to the integer replay of tests/adaptive_ref.py: everything in the adaptive loop is integer, so
after every step the list (ascending), every record's 64 bytes, the count and the sample counter must equal the replay's -- on the BVH
build, the flat scan (MIRT_FLAG_NO_GRID) and under the Hosek sky.  Then the rule on the device at its corners against
mirt_adapt_active, the sums against mirt_ctx_accum_add and the resolve against mirt_ctx_accum_resolve where every pixel holds the same
count, the resolve against the oracle's resolve_channel where the counts differ, a band and a tile partition (the RNG stream belongs
to the ABSOLUTE pixel), a tree 32 levels deep whose stacks fill, and refusals that leave no trace.  One context for the module."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
import adaptive_ref as ar
import deep_worlds as dw
import hbm_worlds
import oracle_binding as ob
import radiance_frames as rf
import radiance_ref as rr

pytestmark = pytest.mark.gpu

W, H = ar.W, ar.H
NO_GRID, HOSEK = m.MIRT_FLAG_NO_GRID, m.MIRT_FLAG_SKY_HOSEK
LINEAR = m.MIRT_FLAG_NO_TONEMAP | m.MIRT_FLAG_NO_SRGB
ADAPT = (ar.MIN_SAMPLES, ar.MAX_SAMPLES, ar.TOLERANCE)


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _name(hosek, bvh):
    tf = ("false", "true")
    return f"adapt_pixels_kernel<{tf[hosek]},{tf[bvh]}>"


def _same_records(got, want, what):
    assert got.dtype == want.dtype == ADAPT_PIXEL_DTYPE and got.shape == want.shape, what
    bad = np.nonzero((_bytes(got) != _bytes(want)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _step_equals(ctx, p, adapt, want, what, total_before=0):
    """One step on the device against one step of the replay."""
    ctx.adapt_step(p, adapt)
    lst, st = ctx.adapt_list(), ctx.adapt_stats()
    print(f"{what}: {len(lst)} listed, {st['total_samples']} samples so far, {st['kernel_ms']:.3f} ms")
    assert lst.dtype == np.uint32 and (np.diff(lst.astype(np.int64)) > 0).all(), f"{what}: the list is not ascending"
    assert np.array_equal(lst, want["list"]), f"{what}: the list differs from the replay's ({len(lst)} entries, want {len(want['list'])})"
    _same_records(ctx.adapt_read(), want["records"], what)
    assert st["active"] == len(want["list"]) and st["total_samples"] == total_before + want["total"], (what, st)
    return st


def _loop(ctx, p, steps, what):
    adapt = m.make_adapt_params(*ADAPT)
    ctx.adapt_reset(p)
    st0 = ctx.adapt_stats()
    assert (st0["pixels"], st0["active"], st0["steps"], st0["total_samples"]) == (len(steps[0]["records"]), 0, 0, 0)
    assert not _bytes(ctx.adapt_read()).any()
    for k, want in enumerate(steps):
        st = _step_equals(ctx, p, adapt, want, f"{what}, step {k + 1}")
        assert st["steps"] == k + 1 and st["kernel_ms"] > 0.0


# ---- 1. the whole loop ----

def test_the_whole_loop_on_the_bvh_build(ctx):
    steps = ar.reference_loop()
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params()
    _loop(ctx, p, steps, "BVH build")
    assert ctx.last_kernel() == _name(False, True)
    # the ninth step changed nothing
    assert len(steps[-1]["list"]) == 0
    _same_records(steps[-1]["records"], steps[-2]["records"], "the replay's ninth step")
    final = ctx.adapt_read()["samples"]
    assert [int((final == n).sum()) for n in range(4, 33, 4)] == [805, 132, 113, 85, 68, 60, 30, 243]


def test_three_steps_on_the_flat_scan(ctx):
    ctx.set_scene(ar.scene(), hbm=True, bvh="device")
    _loop(ctx, ar.params(flags=NO_GRID), ar.reference_loop()[:3], "MIRT_FLAG_NO_GRID")
    assert ctx.last_kernel() == _name(False, False)


def test_three_steps_under_the_hosek_sky(ctx):
    sd = ar.scene(rr.sky_blob())
    p = ar.params(flags=HOSEK)
    frames = ar.sample_frames(sd, p, 3 * ar.SPP, "field300")
    assert not np.array_equal(frames, ar.sample_frames(ar.scene(), ar.params(), 3 * ar.SPP, "field300"))       # another sky, other sums
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert len(steps[1]["list"]) % 64 != 0 and 0 < len(steps[2]["list"]) < len(steps[1]["list"])
    ctx.set_scene(sd, hbm=True)
    _loop(ctx, p, steps, "MIRT_FLAG_SKY_HOSEK")
    assert ctx.last_kernel() == _name(True, True)
    _loop(ctx, ar.params(flags=HOSEK | NO_GRID), steps, "MIRT_FLAG_SKY_HOSEK | MIRT_FLAG_NO_GRID")
    assert ctx.last_kernel() == _name(True, False)


# ---- 2. the rule on the device at its corners ----

def test_the_rule_on_the_device_at_its_corners(ctx):
    recs, cases = ar.corner_records()
    w, h = 64, 2
    assert len(recs) == w * h
    ctx.set_scene(ar.scene(w=w, h=h), hbm=True)
    p = ar.params(w=w, h=h)
    ctx.adapt_reset(p)
    for case in cases:
        adapt = m.make_adapt_params(*case)
        want = m.adapt_active(recs, adapt)
        assert np.array_equal(want, [ar.record_active(r, *case) for r in recs])
        ctx.adapt_write(recs)
        _same_records(ctx.adapt_read(), recs, "write then read")
        ctx.adapt_step(p, adapt)
        lst, after = ctx.adapt_list(), ctx.adapt_read()
        assert np.array_equal(lst, np.nonzero(want)[0]), f"(min, max, tolerance) = {case}: the device lists {lst.tolist()}, the host rule {np.nonzero(want)[0].tolist()}"
        _same_records(after[~want], recs[~want], f"{case}: records that were not listed")
        assert (after["samples"][want] == recs["samples"][want] + ar.SPP).all() and not after["_pad0"].any() and not after["_pad1"].any()
        assert (after["sum"][want] >= recs["sum"][want]).all() and (after["even"][want] >= recs["even"][want]).all()


# ---- 3. against what exists, and 4. the resolve ----

def test_every_pixel_in_every_step_equals_the_accumulation(ctx):
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params()
    adapt = m.make_adapt_params(16, 16, 0)
    ctx.adapt_reset(p)
    ctx.accum_reset(p)
    for k in range(4):
        ctx.adapt_step(p, adapt)
        assert ctx.adapt_stats()["active"] == W * H
        ctx.accum_add(p)
    ctx.adapt_step(p, adapt)
    st = ctx.adapt_stats()
    assert (st["active"], st["steps"], st["total_samples"]) == (0, 5, 16 * W * H)
    recs = ctx.adapt_read()
    assert ctx.accum_samples() == 16 and (recs["samples"] == 16).all()
    assert np.array_equal(recs["sum"], ctx.accum_read(p).reshape(-1, 3)), "sum != mirt_ctx_accum_add x 4"
    frames = ar.sample_frames(ar.scene(), p, 16, "field300")
    assert np.array_equal(recs["even"], frames[0::2].sum(axis=0, dtype=np.uint64)) and np.array_equal(recs["sum"], frames.sum(axis=0, dtype=np.uint64))
    for flags in (0, m.MIRT_FLAG_NO_TONEMAP, m.MIRT_FLAG_NO_SRGB, LINEAR):
        q = ar.params(flags=flags)
        got, want = ctx.adapt_resolve(q), ctx.accum_resolve(q)
        assert got.shape == (H, W, 4) and np.array_equal(got, want), f"flags {flags:#x}: adapt_resolve != accum_resolve on {int((got != want).any(2).sum())} pixels"


def test_resolve_with_unequal_counts(ctx):
    steps = ar.reference_loop()
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params()
    with pytest.raises(m.MirtError) as e:                       # before the first step: nothing to resolve
        ctx.adapt_reset(p)
        ctx.adapt_resolve(p)
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    adapt = m.make_adapt_params(*ADAPT)                         # the finished loop of the first test, run again on the device
    for _ in steps:
        ctx.adapt_step(p, adapt)
    recs = ctx.adapt_read()
    _same_records(recs, steps[-1]["records"], "the finished loop")
    assert len(np.unique(recs["samples"])) == 8
    for flags in (0, m.MIRT_FLAG_NO_TONEMAP, m.MIRT_FLAG_NO_SRGB, LINEAR):
        got = ctx.adapt_resolve(ar.params(flags=flags)).reshape(-1, 4)
        assert (got[:, 3] == 255).all()
        for n in np.unique(recs["samples"]):
            sel = recs["samples"] == n
            want = ob.resolve_channel(recs["sum"][sel], int(n), flags)
            assert np.array_equal(got[sel, :3], want), f"flags {flags:#x}, pixels of {n} samples: {int((got[sel, :3] != want).any(1).sum())} of {int(sel.sum())} differ"
    # a pixel without samples is black, A = 255; the device form writes the same bytes
    holes = recs.copy()
    holes[5:9] = np.zeros(4, ADAPT_PIXEL_DTYPE)
    ctx.adapt_write(holes)
    host = ctx.adapt_resolve(p)
    assert (host.reshape(-1, 4)[5:9] == (0, 0, 0, 255)).all()
    import torch
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.adapt_resolve_device(p, out.data_ptr())
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)


# ---- 5. a band ----

@pytest.mark.parametrize("rows", [dict(row_begin=8, row_end=24), dict(row_begin=8, row_end=24, tile_rows=4, n_parts=2, part=1)],
                         ids=["band", "tile partition"])
def test_a_band_keeps_the_absolute_pixels_streams(ctx, rows):
    p = ar.params(**rows)
    n_rows = m.params_out_rows(p)
    assert n_rows == (16 if "tile_rows" not in rows else 8)
    frames = ar.sample_frames(ar.scene(), p, 3 * ar.SPP, "field300")
    whole = ar.sample_frames(ar.scene(), ar.params(), 3 * ar.SPP, "field300").reshape(-1, H, W, 3)
    picked = np.stack([whole[:, m.params_out_row_index(p, i)] for i in range(n_rows)], 1).reshape(len(whole), -1, 3)
    assert np.array_equal(frames, picked)                       # the oracle's band is the whole frame's rows ...
    assert not np.array_equal(frames, whole[:, :n_rows].reshape(len(whole), -1, 3))      # ... and not the rows a band-relative index would take
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert 0 < len(steps[2]["list"]) < len(steps[1]["list"]) < n_rows * W
    ctx.set_scene(ar.scene(), hbm=True)
    _loop(ctx, p, steps, f"rows {rows}")


# ---- 6. full stacks ----

def _deepest_small_world():
    """The smallest world of tests/deep_worlds.py whose tree is 32 levels deep, with the view that fills its stacks."""
    deep = [n for n in list(dw.LINES) + list(dw.STAIRS) if (dw.DEVICE_DEPTH[n] if n in dw.STAIRS else dw.HOST_DEPTH[n]) == 32]
    name = min(deep, key=lambda n: len(dw.ray_set(n)[0]))
    view = list(rf.deep_cameras(name))[-1]
    return name, view


def test_full_stacks_on_a_tree_32_deep(ctx):
    name, view = _deepest_small_world()
    cam = rf.deep_cameras(name)[view]
    ctx.set_scene(rf.deep_scene(name, cam), hbm=True, bvh="device" if name in dw.STAIRS else "host")
    assert ctx.bvh_info()["plan"]["max_depth"] == 32 == m.MIRT_BVH_MAX_DEPTH
    w, h = rf.DEEP_W, rf.DEEP_H
    adapt = m.make_adapt_params(4, 8, 256)
    after = {}
    for flags in (0, NO_GRID):
        p = ar.params(w=w, h=h, flags=flags, bounces=6)
        ctx.adapt_reset(p)
        lists = []
        for _ in range(2):
            ctx.adapt_step(p, adapt)
            lists.append(ctx.adapt_list())
        assert ctx.last_kernel() == _name(False, flags == 0)
        after[flags] = (lists, ctx.adapt_read())
    assert len(after[0][0][0]) == w * h and 0 < len(after[0][0][1]) < w * h
    for a, b in zip(after[0][0], after[NO_GRID][0]):
        assert np.array_equal(a, b), f"{name}: the BVH build lists other pixels than the flat scan"
    _same_records(after[0][1], after[NO_GRID][1], f"{name} ({view}): BVH build against MIRT_FLAG_NO_GRID")
    # ... and both are the oracle's
    frames = ar.sample_frames(rf.deep_scene(name, cam), ar.params(w=w, h=h, bounces=6), 8, name + view)
    _same_records(after[0][1], ar.replay(frames, ar.SPP, 4, 8, 256, 2)[-1]["records"], f"{name} ({view}): against the replay")


# ---- 7. refusals leave no trace ----

def test_refusals_leave_no_trace(ctx):
    lib = m.lib()
    ctx.set_scene(ar.scene(), hbm=True)
    p, adapt = ar.params(), m.make_adapt_params(*ADAPT)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    accum_before, stats_before = ctx.accum_read(p).copy(), ctx.stats()
    ctx.adapt_reset(p)
    ctx.adapt_step(p, adapt)
    ctx.adapt_step(p, adapt)
    before, list_before, st_before = ctx.adapt_read(), ctx.adapt_list(), ctx.adapt_stats()
    kernel_before = ctx.last_kernel()

    def refused(params, ad, code, what):
        rc = lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(params), C.byref(ad), None)
        assert rc == code, f"{what}: {_abi.STATUS.get(rc, rc)} ({lib.mirt_last_error().decode()})"
        _same_records(ctx.adapt_read(), before, what)
        st = ctx.adapt_stats()
        assert np.array_equal(ctx.adapt_list(), list_before) and (st["steps"], st["total_samples"], st["active"]) == \
            (st_before["steps"], st_before["total_samples"], st_before["active"]), what
        assert ctx.last_kernel() == kernel_before

    bad_flags = m.make_adapt_params(*ADAPT)
    bad_flags.flags = 1
    refused(ar.params(spp=3), adapt, _abi.MIRT_ERR_SPP_RANGE, "odd spp")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PT, seed=ar.SEED, frame_spp=2), adapt, _abi.MIRT_ERR_FRAME_SPP, "frame_spp != 0")
    refused(p, bad_flags, _abi.MIRT_ERR_BAD_MODE, "adapt->flags != 0")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_WORK")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_GRID")
    refused(ar.params(w=W + 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another width")
    refused(ar.params(row_begin=0, row_end=H - 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another row count")
    refused(ar.params(spp=0), adapt, _abi.MIRT_ERR_SPP_ZERO, "spp == 0")
    refused(ar.params(flags=HOSEK), adapt, _abi.MIRT_ERR_SKY, "MIRT_FLAG_SKY_HOSEK without a blob")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PARITY), adapt, _abi.MIRT_ERR_BAD_MODE, "parity mode")
    refused(p, m.make_adapt_params(4, _abi.MIRT_MAX_SPP_PER_CALL + 1, 4096), _abi.MIRT_ERR_SPP_RANGE, "max_samples above the per-call limit")
    assert lib.mirt_ctx_adapt_step_device(ctx._h, None, C.byref(adapt), None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(p), None, None) == _abi.MIRT_ERR_NULL_POINTER
    # the blocking calls' own refusals
    n, small = C.c_uint32(), np.zeros(4, np.uint32)
    assert lib.mirt_ctx_adapt_list_read(ctx._h, C.c_void_p(small.ctypes.data), 4, C.byref(n)) == _abi.MIRT_ERR_OUT_BUFFER and n.value == len(list_before)
    assert lib.mirt_ctx_adapt_read(ctx._h, C.c_void_p(small.ctypes.data), 4) == _abi.MIRT_ERR_OUT_BUFFER
    assert lib.mirt_ctx_adapt_write(ctx._h, C.c_void_p(small.ctypes.data), 4) == _abi.MIRT_ERR_OUT_BUFFER
    assert lib.mirt_ctx_adapt_resolve(ctx._h, C.byref(p), C.c_void_p(small.ctypes.data), 16) == _abi.MIRT_ERR_OUT_BUFFER
    _same_records(ctx.adapt_read(), before, "after the blocking calls' refusals")
    # successful steps touched neither the accumulation nor MirtStats
    assert np.array_equal(ctx.accum_read(p), accum_before) and ctx.accum_samples() == 4
    stats_after = ctx.stats()
    assert stats_after["launches"] == 0 and stats_after["samples"] == stats_before["samples"] and stats_after["kernel_ms"] == stats_before["kernel_ms"]
    # no MIRT_SCENE_HBM scene: an LDS scene refuses the step, and a fresh context too
    ctx.set_scene(ar.scene())
    refused(p, adapt, _abi.MIRT_ERR_NO_SCENE, "an LDS scene")
    with m.Context(0) as fresh:
        assert lib.mirt_ctx_adapt_step_device(fresh._h, C.byref(p), C.byref(adapt), None) == _abi.MIRT_ERR_NO_SCENE
        assert lib.mirt_ctx_adapt_list_read(fresh._h, C.c_void_p(small.ctypes.data), 4, C.byref(n)) == _abi.MIRT_ERR_NO_SCENE
        assert lib.mirt_ctx_adapt_read(fresh._h, C.c_void_p(small.ctypes.data), 4) == _abi.MIRT_ERR_NO_SCENE
        assert fresh.adapt_stats() == {"pixels": 0, "total_samples": 0, "active": 0, "steps": 0, "kernel_ms": 0.0}


def test_raytracer_render_adaptive():
    """The host object: steps until nothing is active -> the image and the sample-count map, equal to the loop driven by hand."""
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(W, H), sampling=m.SamplingParams(max_samples_per_pixel=32, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        img, counts = rt.render_adaptive(4096, 32, seed=3)
        assert img.shape == (H, W, 4) and counts.shape == (H, W) and counts.dtype == np.uint32
        assert counts.min() >= 4 and counts.max() <= 32 and (counts % 4 == 0).all() and len(np.unique(counts)) > 2
        c = rt._ctx
        recs, adapt = c.adapt_read(), m.make_adapt_params(4, 32, 4096)
        assert np.array_equal(recs["samples"].reshape(H, W), counts) and not m.adapt_active(recs, adapt).any()
        assert c.adapt_stats()["total_samples"] == int(counts.sum())
        with pytest.raises(ValueError):
            rt.render_adaptive(4096, 32, step=3)
    finally:
        rt.close()
