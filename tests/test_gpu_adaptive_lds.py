"""MIRT_ADAPT_LDS on the device: adaptive steps and runs on a scene that stays in LDS (adapt_pixels_lds_kernel<HOSEK,GRID> and its run
build) must leave the list, the count, the 64-bit sample counter, the run log and all 64 bytes of every record exactly as the integer
replay of tests/adaptive_ref.py / adaptive_run_ref.py has them -- and as the same call leaves them on a context that holds the world as a
MIRT_SCENE_HBM scene.  The frame is 48 x 32: six blocks, 24 waves.  The shapes are the smallest at which this kernel can go wrong: both
layouts, both skies, every g (forced, chosen by the device, capped by spp 2 and 6), waves that stride over six units, waves without a
unit in a live block, lists of 70 and of 1, bands and a tile partition, a scene without a grid, and the largest blob LDS takes."""
import ctypes as C
import functools

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
import adaptive_lds_ref as lr
import adaptive_ref as ar
import adaptive_run_ref as rr
import helpers
import radiance_ref as rad

pytestmark = pytest.mark.gpu

W, H = ar.W, ar.H
NO_GRID, HOSEK = m.MIRT_FLAG_NO_GRID, m.MIRT_FLAG_SKY_HOSEK
LINEAR = m.MIRT_FLAG_NO_TONEMAP | m.MIRT_FLAG_NO_SRGB
ADAPT = (ar.MIN_SAMPLES, ar.MAX_SAMPLES, ar.TOLERANCE)
TF = ("false", "true")
LAUNCH_WAVES = 4 * (W * H // 256)               # the default launch of this frame: ceil(1536 / 256) = 6 blocks of four waves


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _name(hosek, grid, run=False):
    return f"adapt_pixels_lds{'_run' if run else ''}_kernel<{TF[bool(hosek)]},{TF[bool(grid)]}>"


def _lds(*case, pool=False):
    return m.make_adapt_params(*case, pool=pool, lds=True)


def _same_records(got, want, what):
    assert got.dtype == want.dtype == ADAPT_PIXEL_DTYPE and got.shape == want.shape, what
    bad = np.nonzero((_bytes(got) != _bytes(want)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _step_equals(ctx, p, adapt, want, what, total_before=0):
    """One step on the device against one step of the replay."""
    ctx.adapt_step(p, adapt)
    lst, st = ctx.adapt_list(), ctx.adapt_stats()
    print(f"{what}: {ctx.last_kernel()}, {len(lst)} listed, {st['total_samples']} samples so far, {st['kernel_ms']:.3f} ms")
    assert lst.dtype == np.uint32 and (np.diff(lst.astype(np.int64)) > 0).all(), f"{what}: the list is not ascending"
    assert np.array_equal(lst, want["list"]), f"{what}: the list differs from the replay's ({len(lst)} entries, want {len(want['list'])})"
    _same_records(ctx.adapt_read(), want["records"], what)
    assert st["active"] == len(want["list"]) and st["total_samples"] == total_before + want["total"], (what, st)
    return st


def _loop(ctx, p, steps, what, case=ADAPT):
    adapt = _lds(*case)
    ctx.adapt_reset(p)
    assert not _bytes(ctx.adapt_read()).any()
    for k, want in enumerate(steps):
        st = _step_equals(ctx, p, adapt, want, f"{what}, step {k + 1}")
        assert st["steps"] == k + 1 and st["kernel_ms"] > 0.0


@functools.lru_cache(maxsize=None)
def _hosek_steps():
    frames = ar.sample_frames(ar.scene(rad.sky_blob()), ar.params(flags=HOSEK), 3 * ar.SPP, "field300")
    assert not np.array_equal(frames, ar.sample_frames(ar.scene(), ar.params(), 3 * ar.SPP, "field300"))       # another sky, other sums
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert len(steps[1]["list"]) % 64 != 0 and 0 < len(steps[2]["list"]) < len(steps[1]["list"])
    return tuple(steps)


@functools.lru_cache(maxsize=None)
def _steps_of(spp):
    """Three steps of `spp` samples on the whole-loop input."""
    frames = ar.sample_frames(ar.scene(), ar.params(), ar.MAX_SAMPLES + ar.SPP, "field300")
    steps = ar.replay(frames, spp, *ADAPT, 3)
    assert len(steps[2]["list"]) > 0
    return tuple(steps)


# ---- 1. the whole loop, grid build ----

def test_the_whole_loop_on_the_grid_build(ctx):
    steps = ar.reference_loop()
    ctx.set_scene(ar.scene())                                   # in LDS: without the flag the step is refused (test_gpu_adaptive.py)
    _loop(ctx, ar.params(), steps, "grid build")
    assert ctx.last_kernel() == _name(False, True)
    final = ctx.adapt_read()["samples"]
    assert [int((final == n).sum()) for n in range(4, 33, 4)] == [805, 132, 113, 85, 68, 60, 30, 243]
    with pytest.raises(m.MirtError) as e:                       # the scene did not move
        ctx.bvh_info()
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE


# ---- 2. the other builds ----

def test_three_steps_on_the_flat_layout(ctx):
    ctx.set_scene(ar.scene())
    _loop(ctx, ar.params(flags=NO_GRID), ar.reference_loop()[:3], "MIRT_FLAG_NO_GRID")
    assert ctx.last_kernel() == _name(False, False)


def test_three_steps_under_the_hosek_sky_in_both_layouts(ctx):
    steps = _hosek_steps()
    ctx.set_scene(ar.scene(rad.sky_blob()))
    _loop(ctx, ar.params(flags=HOSEK), steps, "MIRT_FLAG_SKY_HOSEK")
    assert ctx.last_kernel() == _name(True, True)
    _loop(ctx, ar.params(flags=HOSEK | NO_GRID), steps, "MIRT_FLAG_SKY_HOSEK | MIRT_FLAG_NO_GRID")
    assert ctx.last_kernel() == _name(True, False)
    # MIRT_ADAPT_POOL on a scene in LDS: a hint that is ignored
    adapt = _lds(*ADAPT, pool=True)
    ctx.adapt_reset(ar.params(flags=HOSEK))
    _step_equals(ctx, ar.params(flags=HOSEK), adapt, steps[0], "MIRT_ADAPT_POOL | MIRT_ADAPT_LDS")
    assert ctx.last_kernel() == _name(True, True)


# ---- 3. groups ----

def test_the_device_chooses_the_groups_of_the_default_launch():
    """The default launch of this frame is six blocks, 24 waves: the first step's 24 units of 64 give every wave one (g = 0), and every
    later list is too short for that, so that the device deals the samples to four groups (g = 2): the loop of test 1 runs both."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count >= W * H // 256      # the CUs x blocks_per_cu bound does not bind
    counts = [len(s["list"]) for s in ar.reference_loop()]
    assert counts[0] == W * H and LAUNCH_WAVES == 24
    want = [m.adapt_lds_groups(c, ar.SPP, LAUNCH_WAVES) for c in counts]
    assert want == [0] + [2] * (len(counts) - 2) + [0] and all(-(-c // 64) < LAUNCH_WAVES for c in counts[1:])
    assert m.adapt_lds_groups(counts[1], 2, LAUNCH_WAVES) == 1 == m.adapt_lds_groups(counts[1], 6, LAUNCH_WAVES)       # spp 2 and 6 cap g at 1


@pytest.mark.parametrize("knob", ["1", "2", "3"])
def test_forced_groups_leave_the_same_bytes(monkeypatch, knob):
    monkeypatch.setenv("MIRT_ADAPT_LDS_GROUPS", knob)                  # read when a context is created
    with m.Context(0) as own:
        own.set_scene(ar.scene())
        _loop(own, ar.params(), ar.reference_loop()[:3], f"MIRT_ADAPT_LDS_GROUPS={knob}, grid build")
        _loop(own, ar.params(flags=NO_GRID), ar.reference_loop()[:3], f"MIRT_ADAPT_LDS_GROUPS={knob}, flat layout")
        if knob == "3":                                                # the forced g = 2 is still capped by spp: 1 for 2 and for 6 (shares of 3)
            for spp in (2, 6):
                _loop(own, ar.params(spp=spp), _steps_of(spp), f"MIRT_ADAPT_LDS_GROUPS=3, spp {spp}")


@pytest.mark.parametrize("spp", [2, 6])
def test_spp_caps_the_groups_the_device_chooses(ctx, spp):
    ctx.set_scene(ar.scene())
    _loop(ctx, ar.params(spp=spp), _steps_of(spp), f"spp {spp}")
    _loop(ctx, ar.params(spp=spp, flags=NO_GRID), _steps_of(spp), f"spp {spp}, flat layout")


# ---- 4. striding and idle waves ----

def _few_active(steps, n_active):
    """The records after the loop's second step with exactly n_active pixels left active: the others hold max_samples."""
    recs = steps[1]["records"].copy()
    active = np.nonzero([ar.record_active(r, *ADAPT) for r in recs])[0]
    assert len(active) > 70
    keep = active[:: len(active) // n_active][:n_active]
    assert len(keep) == n_active
    off = np.setdiff1d(np.arange(len(recs)), keep)
    recs["samples"][off] = ar.MAX_SAMPLES
    assert int(np.sum([ar.record_active(r, *ADAPT) for r in recs])) == n_active
    return recs


def test_one_block_strides_over_the_units_and_idle_waves_pass(monkeypatch):
    monkeypatch.setenv("MIRT_ADAPT_LDS_BLOCKS", "1")                   # read when a context is created: four waves in all
    steps = ar.reference_loop()
    assert m.adapt_lds_groups(W * H, ar.SPP, 4) == 0 and W * H // 64 == 6 * 4      # step 1: every wave serves six units
    frames = ar.sample_frames(ar.scene(), ar.params(), ar.MAX_SAMPLES + ar.SPP, "field300")
    with m.Context(0) as own:
        own.set_scene(ar.scene())
        for flags in (0, NO_GRID):
            p = ar.params(flags=flags)
            _loop(own, p, steps, f"one block, flags {flags:#x}")
            for n_active, g, units in ((70, 2, 5), (1, 2, 1)):          # five units for four waves; one unit: three waves idle in a live block
                assert m.adapt_lds_groups(n_active, ar.SPP, 4) == g and -(-n_active // (64 >> g)) == units
                start = _few_active(steps, n_active)
                want = ar.replay(frames, ar.SPP, *ADAPT, 1, start=start)[0]
                assert len(want["list"]) == n_active
                own.adapt_reset(p)
                own.adapt_write(start)
                _step_equals(own, p, _lds(*ADAPT), want, f"one block, {n_active} active, flags {flags:#x}")
                after = own.adapt_read()
                unlisted = np.setdiff1d(np.arange(W * H), want["list"])
                _same_records(after[unlisted], start[unlisted], f"{n_active} active: the records that were not listed")


# ---- 5. runs ----

RUN = (10, 3000, 16)                                                   # base 2 grown to a cap of 16


@functools.lru_cache(maxsize=None)
def _reference_run():
    want = rr.replay_run(rr.frames_of(), 2, *ADAPT, RUN)
    sizes = [int(s) for _, s in want["log"]]
    assert sizes[0] == 2 and 16 in sizes and len({s for s in sizes if s}) >= 3, want["log"].tolist()      # grown from the base to the cap
    return want


def _run_state(ctx, p, adapt, run):
    ctx.adapt_reset(p)
    ctx.adapt_run(p, adapt, m.make_adapt_run(*run))
    st = ctx.adapt_stats()
    return {"log": ctx.adapt_run_log(), "list": ctx.adapt_list(), "records": ctx.adapt_read(), "total": st["total_samples"], "active": st["active"],
            "steps": st["steps"], "kernel": ctx.last_kernel()}


@pytest.mark.parametrize("flags", [0, NO_GRID], ids=["grid", "flat"])
def test_a_run_equals_the_replay_and_the_same_run_on_an_hbm_scene(ctx, flags):
    want = _reference_run()
    p = ar.params(spp=2, flags=flags)
    ctx.set_scene(ar.scene())
    got = _run_state(ctx, p, _lds(*ADAPT), RUN)
    print(f"run, flags {flags:#x}: {got['kernel']}, log {got['log'].tolist()}")
    assert got["kernel"] == _name(False, flags == 0, run=True)
    assert got["log"].dtype == np.uint32 and np.array_equal(got["log"], want["log"]), (got["log"].tolist(), want["log"].tolist())
    last = want["steps"][-1]
    assert got["total"] == last["total"] and got["steps"] == RUN[0] and got["active"] == int(want["log"][-1][0]) == len(got["list"])
    if last["list"] is not None:
        assert np.array_equal(got["list"], last["list"])
    _same_records(got["records"], last["records"], f"run, flags {flags:#x}")
    with m.Context(0) as hbm:                                           # the same world as a MIRT_SCENE_HBM scene; the flag is ignored there
        hbm.set_scene(ar.scene(), hbm=True)
        other = _run_state(hbm, p, _lds(*ADAPT), RUN)
        assert other["kernel"] == f"adapt_pixels_run_kernel<false,{TF[flags == 0]}>"
    assert np.array_equal(got["log"], other["log"]) and np.array_equal(got["list"], other["list"]) and got["total"] == other["total"]
    _same_records(got["records"], other["records"], f"run, flags {flags:#x}: LDS against HBM")


# ---- 6. bands ----

@pytest.mark.parametrize("rows", [dict(row_begin=8, row_end=24), dict(row_begin=8, row_end=24, tile_rows=4, n_parts=2, part=1)],
                         ids=["band", "tile partition"])
def test_a_band_keeps_the_absolute_pixels_streams(ctx, rows):
    p = ar.params(**rows)
    n_rows = m.params_out_rows(p)
    assert n_rows == (16 if "tile_rows" not in rows else 8)
    frames = ar.sample_frames(ar.scene(), p, 3 * ar.SPP, "field300")
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert 0 < len(steps[2]["list"]) < len(steps[1]["list"]) < n_rows * W
    ctx.set_scene(ar.scene())
    _loop(ctx, p, steps, f"rows {rows}")
    _loop(ctx, ar.params(flags=NO_GRID, **rows), steps, f"rows {rows}, flat layout")


# ---- 7. against the accumulation ----

def test_every_pixel_in_every_step_equals_the_accumulation(ctx):
    ctx.set_scene(ar.scene())
    p = ar.params()
    adapt = _lds(16, 16, 0)
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
    assert np.array_equal(recs["sum"], ctx.accum_read(p).reshape(-1, 3)), "sum != mirt_ctx_accum_add x 4 on the same LDS context"
    frames = ar.sample_frames(ar.scene(), p, 16, "field300")
    assert np.array_equal(recs["even"], frames[0::2].sum(axis=0, dtype=np.uint64))
    for flags in (0, m.MIRT_FLAG_NO_TONEMAP, m.MIRT_FLAG_NO_SRGB, LINEAR):
        q = ar.params(flags=flags)
        got, want = ctx.adapt_resolve(q), ctx.accum_resolve(q)
        assert got.shape == (H, W, 4) and np.array_equal(got, want), f"flags {flags:#x}: adapt_resolve != accum_resolve on {int((got != want).any(2).sum())} pixels"


# ---- 8. a scene without a grid ----

def test_the_five_sphere_scene_runs_the_flat_build_without_the_flag_no_grid(ctx):
    w, h = 16, 8
    sd = helpers.scene_data("main_rs_scene", w, h)
    p = ar.params(w=w, h=h)
    frames = ar.sample_frames(sd, p, 3 * ar.SPP, "main_rs_scene")
    steps = ar.replay(frames, ar.SPP, *ADAPT, 3)
    assert len(steps[0]["list"]) == w * h and 0 < len(steps[2]["list"]) < w * h
    ctx.set_scene(sd)
    _loop(ctx, p, steps, "main.rs scene")
    assert ctx.last_kernel() == _name(False, False)


# ---- 9. a grid-only world ----

def test_a_grid_only_world_equals_the_hbm_step_and_has_no_flat_build(ctx):
    sd = lr.grid_only_scene()
    p = ar.params()
    adapt = _lds(*ADAPT)
    ctx.set_scene(sd)
    ctx.adapt_reset(p)
    ctx.adapt_step(p, adapt)
    assert ctx.last_kernel() == _name(False, True)
    got, lst, st = ctx.adapt_read(), ctx.adapt_list(), ctx.adapt_stats()
    assert (st["active"], st["total_samples"]) == (W * H, ar.SPP * W * H) and (got["samples"] == ar.SPP).all() and got["sum"].any()
    with m.Context(0) as hbm:
        hbm.set_scene(sd, hbm=True)
        hbm.adapt_reset(p)
        hbm.adapt_step(p, adapt)
        assert hbm.last_kernel() == "adapt_pixels_kernel<false,true>"
        assert np.array_equal(lst, hbm.adapt_list())
        _same_records(got, hbm.adapt_read(), "grid-only world: LDS against HBM")
    # MIRT_FLAG_NO_GRID asks for the flat layout, which this world does not have
    rc = m.lib().mirt_ctx_adapt_step_device(ctx._h, C.byref(ar.params(flags=NO_GRID)), C.byref(adapt), None)
    assert rc == _abi.MIRT_ERR_SCENE_TOO_LARGE, _abi.STATUS.get(rc, rc)
    st2 = ctx.adapt_stats()
    assert (st2["steps"], st2["total_samples"], st2["active"]) == (st["steps"], st["total_samples"], st["active"]) and ctx.last_kernel() == _name(False, True)
    assert np.array_equal(ctx.adapt_list(), lst)
    _same_records(ctx.adapt_read(), got, "after the refused MIRT_FLAG_NO_GRID step")


# ---- 10. refusals and state ----

def test_refusals_leave_no_trace_and_steps_leave_the_other_state_alone(ctx):
    lib = m.lib()
    ctx.set_scene(ar.scene())
    p, adapt = ar.params(), _lds(*ADAPT)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    accum_before, stats_before = ctx.accum_read(p).copy(), ctx.stats()
    ctx.adapt_reset(p)
    ctx.adapt_step(p, adapt)
    ctx.adapt_step(p, adapt)
    before, list_before, st_before = ctx.adapt_read(), ctx.adapt_list(), ctx.adapt_stats()
    kernel_before = ctx.last_kernel()
    assert kernel_before == _name(False, True)

    def refused(params, ad, code, what):
        rc = lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(params), C.byref(ad), None)
        assert rc == code, f"{what}: {_abi.STATUS.get(rc, rc)} ({lib.mirt_last_error().decode()})"
        run = m.make_adapt_run(3, 0, 0)
        assert lib.mirt_ctx_adapt_run_device(ctx._h, C.byref(params), C.byref(ad), C.byref(run), None) == code, f"{what}: a run"
        _same_records(ctx.adapt_read(), before, what)
        st = ctx.adapt_stats()
        assert np.array_equal(ctx.adapt_list(), list_before) and (st["steps"], st["total_samples"], st["active"]) == \
            (st_before["steps"], st_before["total_samples"], st_before["active"]), what
        assert ctx.last_kernel() == kernel_before

    def flagged(bits):
        a = m.make_adapt_params(*ADAPT)
        a.flags = bits
        return a

    refused(p, m.make_adapt_params(*ADAPT), _abi.MIRT_ERR_NO_SCENE, "an LDS scene without the flag")
    refused(p, flagged(m.MIRT_ADAPT_POOL), _abi.MIRT_ERR_NO_SCENE, "an LDS scene with MIRT_ADAPT_POOL alone")
    refused(p, flagged(8 | 4), _abi.MIRT_ERR_BAD_MODE, "flags 8 | 4")
    refused(p, flagged(8 | 1), _abi.MIRT_ERR_BAD_MODE, "flags 8 | 1")
    refused(p, flagged(8 | 16), _abi.MIRT_ERR_BAD_MODE, "flags 8 | 16")
    # test_gpu_adaptive.py's list, with the flag set
    refused(ar.params(spp=3), adapt, _abi.MIRT_ERR_SPP_RANGE, "odd spp")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PT, seed=ar.SEED, frame_spp=2), adapt, _abi.MIRT_ERR_FRAME_SPP, "frame_spp != 0")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_WORK")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID), adapt, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_GRID")
    refused(ar.params(w=W + 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another width")
    refused(ar.params(row_begin=0, row_end=H - 1), adapt, _abi.MIRT_ERR_OUT_BUFFER, "another row count")
    refused(ar.params(spp=0), adapt, _abi.MIRT_ERR_SPP_ZERO, "spp == 0")
    refused(ar.params(flags=HOSEK), adapt, _abi.MIRT_ERR_SKY, "MIRT_FLAG_SKY_HOSEK without a blob")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PARITY), adapt, _abi.MIRT_ERR_BAD_MODE, "parity mode")
    refused(p, _lds(4, _abi.MIRT_MAX_SPP_PER_CALL + 1, 4096), _abi.MIRT_ERR_SPP_RANGE, "max_samples above the per-call limit")
    assert lib.mirt_ctx_adapt_step_device(ctx._h, None, C.byref(adapt), None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_adapt_step_device(ctx._h, C.byref(p), None, None) == _abi.MIRT_ERR_NULL_POINTER
    with m.Context(0) as fresh:                                         # no scene at all: the flag does not help
        assert lib.mirt_ctx_adapt_step_device(fresh._h, C.byref(p), C.byref(adapt), None) == _abi.MIRT_ERR_NO_SCENE
    # successful steps touched neither the accumulation nor MirtStats
    assert np.array_equal(ctx.accum_read(p), accum_before) and ctx.accum_samples() == 4
    stats_after = ctx.stats()
    assert stats_after["launches"] == 0 and stats_after["samples"] == stats_before["samples"] and stats_after["kernel_ms"] == stats_before["kernel_ms"]
    # a MIRT_SCENE_HBM scene ignores the flag: the same kernel, the same bytes
    ctx.set_scene(ar.scene(), hbm=True)
    seen = {}
    for lds in (False, True):
        for pool in (False, True):
            ctx.adapt_reset(p)
            a = m.make_adapt_params(*ADAPT, pool=pool, lds=lds)
            ctx.adapt_step(p, a)
            ctx.adapt_step(p, a)
            seen[lds, pool] = (ctx.last_kernel(), ctx.adapt_list(), ctx.adapt_read(), ctx.adapt_stats()["total_samples"])
    for pool in (False, True):
        off, on = seen[False, pool], seen[True, pool]
        assert off[0] == on[0] and "lds" not in on[0] and np.array_equal(off[1], on[1]) and off[3] == on[3], (off[0], on[0])
        _same_records(on[2], off[2], f"an HBM scene with the flag, pool {pool}")
    assert seen[True, False][0] == "adapt_pixels_kernel<false,true>" and seen[True, True][0].startswith("adapt_pixels_pool_kernel<")
    _same_records(seen[True, False][2], before, "two steps on the HBM scene against two steps in LDS")


# ---- 11. Raytracer.render_adaptive ----

def test_raytracer_render_adaptive_leaves_the_scene_in_lds():
    scene, cam = m.scenes.three_spheres()

    def tracer():
        rp = m.RenderParams(camera=cam, viewport_size=(W, H), sampling=m.SamplingParams(max_samples_per_pixel=32, num_samples_per_pixel=4, num_bounces=8))
        return m.Raytracer(scene, rp, device=0)

    a, b = tracer(), tracer()
    try:
        img, counts = a.render_adaptive(4096, 32, seed=3, lds=True)
        assert a._ctx.last_kernel() == _name(False, False) and a._hbm is False
        with pytest.raises(m.MirtError) as e:                           # the scene did not move
            a._ctx.bvh_info()
        assert e.value.status == _abi.MIRT_ERR_NO_SCENE
        want_img, want_counts = b.render_adaptive(4096, 32, seed=3)     # the default: the scene becomes an HBM scene
        assert b._hbm is True and "plan" in b._ctx.bvh_info()          # (answers: there is a tree, three spheres deep or not)
        assert len(np.unique(want_counts)) > 2
        assert np.array_equal(counts, want_counts) and np.array_equal(img, want_img)
        img2, counts2 = a.render_adaptive(4096, 32, seed=3, lds=True, run=True)      # a run, on the scene that stayed
        assert a._ctx.last_kernel() == _name(False, False, run=True) and a._hbm is False
        img3, counts3 = b.render_adaptive(4096, 32, seed=3, lds=True)   # an HBM scene: nothing changes
        assert b._ctx.last_kernel() == "adapt_pixels_kernel<false,true>" and np.array_equal(img3, want_img) and np.array_equal(counts3, want_counts)
        want_img2, want_counts2 = b.render_adaptive(4096, 32, seed=3, run=True)
        assert np.array_equal(counts2, want_counts2) and np.array_equal(img2, want_img2)
    finally:
        a.close()
        b.close()
