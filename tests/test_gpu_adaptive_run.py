"""mirt_ctx_adapt_run_device on the device: ONE call queues a whole adaptive loop, and every step's sample count is chosen on the device
from the list the step has just built.  All of it is integer, so the log {count, spp}, the list, the count, the 64-bit sample counter
and all 64 bytes of every record must be those of the integer replay of tests/adaptive_run_ref.py over the CPU oracle's one-sample
frames.  Every case asserts the render kernel's name first -- the run builds have names of their own -- so each fails where a run is not
built.  The shapes are the smallest at which these kernels can go wrong: three step sizes in one run, lists that are multiples of
neither 16 nor 64, pixels that end above max_samples, both parities of a pixel's own sample index under a grown step, lists of 1 to 65
entries, waves that run several grown units, full stacks, a band and a tile partition."""
import ctypes as C
import functools

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
import adaptive_ref as ar
import adaptive_run_ref as rr
import oracle_binding as ob
import radiance_frames as rf
import radiance_ref as rad
import deep_worlds as dw

pytestmark = pytest.mark.gpu

W, H = ar.W, ar.H
NO_GRID, HOSEK = m.MIRT_FLAG_NO_GRID, m.MIRT_FLAG_SKY_HOSEK
ADAPT = (rr.MIN_SAMPLES, rr.MAX_SAMPLES, rr.TOLERANCE)
TF = ("false", "true")
BUILDS = {"bvh": (0, False), "no grid": (NO_GRID, False), "pooled": (0, True)}        # name -> (params.flags, MIRT_ADAPT_POOL)


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _same_records(got, want, what):
    assert got.dtype == want.dtype == ADAPT_PIXEL_DTYPE and got.shape == want.shape, what
    bad = np.nonzero((_bytes(got) != _bytes(want)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _run_name(ctx, flags=0, pool=False, geometry=None):
    """The name of a run's render kernel: adapt_pixels_run_kernel<HOSEK,BVH>, or the pooled run build in the geometry mirt_adapt_pool_plan
    gives for the resident tree."""
    hosek, bvh = bool(flags & HOSEK), not (flags & NO_GRID)
    if not (pool and bvh):
        return f"adapt_pixels_run_kernel<{TF[hosek]},{TF[bvh]}>"
    depth = ctx.bvh_info()["plan"]["max_depth"]
    plan = m.adapt_pool_plan(depth, hosek)
    assert plan["slots"] != 0 and plan["stack_entries"] == depth
    if geometry is not None:
        assert (plan["slots"], plan["waves_per_cu"]) == geometry, (plan, geometry)
    return "adapt_pixels_pool_run_kernel<%d,%d,4,%s>" % (plan["threads"], plan["slots"], TF[hosek])


def _state(ctx):
    st = ctx.adapt_stats()
    return {"list": ctx.adapt_list(), "records": ctx.adapt_read(), "active": st["active"], "total": st["total_samples"], "steps": st["steps"]}


def _run(ctx, p, case, run, name, pool=False, start=None, stream=None, reset=True):
    """(Reset, write `start`,) one run -> the state behind it and its log; the kernel's name first."""
    if reset:
        ctx.adapt_reset(p)
        if start is not None:
            ctx.adapt_write(start)
    ctx.adapt_run(p, m.make_adapt_params(*case, pool=pool), m.make_adapt_run(*run), stream=stream)
    assert ctx.last_kernel() == name, (ctx.last_kernel(), name)
    out = _state(ctx)
    out["log"] = ctx.adapt_run_log()
    return out


def _equals_replay(got, want, what, first_step=0):
    """The state behind a run against replay_run's: the log, the last step's list and count, the counter, every record."""
    log = want["log"][first_step:]
    assert got["log"].dtype == np.uint32 and got["log"].shape == log.shape and np.array_equal(got["log"], log), f"{what}: the log is {got['log'].tolist()}, want {log.tolist()}"
    last = want["steps"][-1]
    assert got["active"] == int(log[-1][0]) == len(got["list"]), (what, got["active"], log[-1].tolist())
    if last["list"] is not None:
        assert got["list"].dtype == np.uint32 and np.array_equal(got["list"], last["list"]), f"{what}: the list differs"
    assert got["total"] == last["total"], (what, got["total"], last["total"])
    _same_records(got["records"], last["records"], what)


@functools.lru_cache(maxsize=None)
def _hosek_reference(name):
    frames = rr.frames_of(rad.sky_blob(), HOSEK)
    assert not np.array_equal(frames, rr.frames_of())
    want = rr.replay_run(frames, rr.BASE, *ADAPT, rr.RUNS[name][0])
    sizes = {int(s) for _, s in want["log"] if s}                # (another image: these runs need not end within max_steps)
    assert len(sizes) >= 2 and want["log"][0].tolist() == [W * H, rr.BASE], want["log"].tolist()
    return want


# ---- 1. the three runs on every build ----

@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", list(rr.RUNS))
def test_the_reference_runs(ctx, name, build):
    want = rr.reference_run(name)
    flags, pool = BUILDS[build]
    ctx.set_scene(ar.scene(), hbm=True)
    run = rr.RUNS[name][0]
    got = _run(ctx, ar.params(flags=flags), ADAPT, run, _run_name(ctx, flags, pool, (112, 16)), pool)
    print(f"{name}, {build}: {ctx.last_kernel()}, log {got['log'].tolist()}")
    _equals_replay(got, want, f"{name}, {build}")
    assert got["steps"] == run[0]
    assert int(got["records"]["samples"].max()) > rr.MAX_SAMPLES or name != "three sizes"


@pytest.mark.parametrize("pool", [False, True], ids=["bvh", "pooled"])
@pytest.mark.parametrize("name", list(rr.RUNS))
def test_the_reference_runs_under_the_hosek_sky(ctx, name, pool):
    want = _hosek_reference(name)
    ctx.set_scene(ar.scene(rad.sky_blob()), hbm=True)
    got = _run(ctx, ar.params(flags=HOSEK), ADAPT, rr.RUNS[name][0], _run_name(ctx, HOSEK, pool, (112, 16)), pool)
    _equals_replay(got, want, f"{name} under the Hosek sky, pooled {pool}")


# ---- 2. a run against the same steps driven by the host ----

@pytest.mark.parametrize("pool", [False, True], ids=["bvh", "pooled"])
def test_a_run_equals_host_driven_steps_of_the_logged_sizes(ctx, pool):
    ctx.set_scene(ar.scene(), hbm=True)
    run = rr.RUNS["three sizes"][0]
    got = _run(ctx, ar.params(), ADAPT, run, _run_name(ctx, 0, pool), pool)
    assert [tuple(e) for e in got["log"].tolist()] == rr.RUNS["three sizes"][1]
    adapt = m.make_adapt_params(*ADAPT, pool=pool)
    ctx.adapt_reset(ar.params())
    for count, spp in got["log"].tolist():
        if spp == 0:
            break
        ctx.adapt_step(ar.params(spp=spp), adapt)
        assert "_run" not in ctx.last_kernel() and ctx.adapt_stats()["active"] == count
    host = _state(ctx)
    _same_records(got["records"], host["records"], "a run against host-driven steps")
    assert got["total"] == host["total"] == 24304


# ---- 3. two runs are one, and 4. the steps behind the empty one ----

@pytest.mark.parametrize("pool", [False, True], ids=["bvh", "pooled"])
def test_a_run_of_three_and_a_run_of_five_are_the_run_of_eight(ctx, pool):
    want = rr.reference_run("three sizes")
    _, min_items, cap = rr.RUNS["three sizes"][0]
    ctx.set_scene(ar.scene(), hbm=True)
    name = _run_name(ctx, 0, pool)
    first = _run(ctx, ar.params(), ADAPT, (3, min_items, cap), name, pool)
    _equals_replay(first, {"log": want["log"][:3], "steps": want["steps"][:3]}, "the first three steps")
    assert first["steps"] == 3 and len(first["list"]) == 540
    rest = _run(ctx, ar.params(), ADAPT, (5, min_items, cap), name, pool, reset=False)
    _equals_replay(rest, want, "five more steps", first_step=3)
    assert rest["steps"] == 8
    # the steps behind the empty one: records, list, count and counter stay, and the log says {0, 0}
    more = _run(ctx, ar.params(), ADAPT, (4, min_items, cap), name, pool, reset=False)
    assert more["log"].tolist() == [[0, 0]] * 4 and more["active"] == 0 and len(more["list"]) == 0
    assert more["total"] == rest["total"] and more["steps"] == 12
    _same_records(more["records"], rest["records"], "a run of empty steps")
    # a shorter log than the run's: refused, and the run's length is reported all the same
    n, small = C.c_uint32(), np.zeros((3, 2), np.uint32)
    assert m.lib().mirt_ctx_adapt_run_read(ctx._h, C.c_void_p(small.ctypes.data), 3, C.byref(n)) == _abi.MIRT_ERR_OUT_BUFFER and n.value == 4
    assert not small.any()


# ---- 5. the identity with a step ----

@pytest.mark.parametrize("build", list(BUILDS))
def test_a_run_of_one_step_that_never_grows_is_a_step(ctx, build):
    flags, pool = BUILDS[build]
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params(flags=flags)
    start = ar.reference_loop()[0]["records"]                   # every pixel at 4 samples: the second step of the host-driven loop
    got = _run(ctx, p, ADAPT, (1, 0, 0), _run_name(ctx, flags, pool), pool, start=start)
    assert got["log"].tolist() == [[731, 4]]
    ctx.adapt_reset(p)
    ctx.adapt_write(start)
    ctx.adapt_step(p, m.make_adapt_params(*ADAPT, pool=pool))
    step = _state(ctx)
    assert np.array_equal(got["list"], step["list"]) and (got["active"], got["total"], got["steps"]) == (step["active"], step["total"], step["steps"]) == (731, 2924, 1)
    _same_records(got["records"], step["records"], f"{build}: a run of one step against a step")
    _same_records(got["records"], ar.reference_loop()[1]["records"], f"{build}: a run of one step against the replay")


# ---- 6. records of the caller's ----

@pytest.mark.parametrize("pool", [False, True], ids=["bvh", "pooled"])
def test_both_parities_of_a_pixels_own_index_meet_a_grown_step(ctx, pool):
    frames = rr.frames_of()
    npix = frames.shape[1]
    n0 = (7 * np.arange(npix)) % 5
    start = np.zeros(npix, ADAPT_PIXEL_DTYPE)
    for n in range(1, 5):
        sel = n0 == n
        start["sum"][sel] = frames[:n, sel].sum(axis=0, dtype=np.uint64)
        start["even"][sel] = frames[0:n:2, sel].sum(axis=0, dtype=np.uint64)
    start["samples"] = n0
    run = (3, 1 << 30, 16)                                      # the cap binds at once: steps of 16 from n0 = 0 .. 4
    want = rr.replay_run(frames, rr.BASE, *ADAPT, run, start=start)
    assert want["log"][0].tolist() == [1380, 16] and want["log"][1][1] == 16 and 0 < want["log"][1][0] < 1380
    first = want["steps"][0]["list"]
    for u in range(0, len(first) - 15, 16):                     # both parities inside every full unit of the first step
        assert len(set((n0[first[u:u + 16]] & 1).tolist())) == 2, u
    ctx.set_scene(ar.scene(), hbm=True)
    got = _run(ctx, ar.params(), ADAPT, run, _run_name(ctx, 0, pool), pool, start=start)
    _equals_replay(got, want, f"records that start at n0 = 7 i mod 5, pooled {pool}")


@pytest.mark.parametrize("pool", [False, True], ids=["bvh", "pooled"])
@pytest.mark.parametrize("k", [1, 15, 16, 17, 63, 64, 65])
def test_small_counts_at_a_grown_step(ctx, k, pool):
    frames = rr.frames_of(n=8)
    npix = W * H
    places = np.sort(np.random.default_rng(100 + k).choice(npix, k, replace=False))
    assert k == 1 or ((np.diff(places) > 1).any() and len(set((places // W).tolist())) > 1)      # scattered, across rows
    start = np.zeros(npix, ADAPT_PIXEL_DTYPE)                   # canaries: every byte of an unlisted record is somebody's
    start["sum"] = (0x0123456789ABCDEF + 3 * np.arange(npix, dtype=np.uint64))[:, None] + np.arange(3, dtype=np.uint64)
    start["even"] = (0x00FEDCBA98765432 + 5 * np.arange(npix, dtype=np.uint64))[:, None] + np.arange(3, dtype=np.uint64)
    start["samples"] = 8
    start["_pad0"], start["_pad1"] = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
    start[places] = np.zeros(k, ADAPT_PIXEL_DTYPE)
    case, run = (8, 8, 0), (1, 1 << 20, 8)                      # base 2 grown to 8 by the device: k x 2, k x 4 are far below 2^20
    want = rr.replay_run(frames, 2, *case, run, start=start)
    assert want["log"].tolist() == [[k, 8]] and np.array_equal(want["steps"][0]["list"], places)
    ctx.set_scene(ar.scene(), hbm=True)
    got = _run(ctx, ar.params(spp=2), case, run, _run_name(ctx, 0, pool), pool, start=start)
    _equals_replay(got, want, f"{k} listed records")
    recs = got["records"]
    assert np.array_equal(recs["sum"][places], frames[0:8, places].sum(axis=0, dtype=np.uint64))
    assert np.array_equal(recs["even"][places], frames[0:8:2, places].sum(axis=0, dtype=np.uint64)) and (recs["samples"][places] == 8).all()
    rest = np.ones(npix, bool)
    rest[places] = False
    _same_records(recs[rest], start[rest], f"{k} listed records: the others")


# ---- 7. several grown units per wave ----

def test_one_block_whose_waves_run_several_grown_units(monkeypatch):
    monkeypatch.setenv("MIRT_ADAPT_POOL_BLOCKS", "1")                  # read when a context is created
    want = rr.reference_run("k jumps by two")
    assert [-(-int(c) // 16) for c, _ in want["log"][:3]] == [96, 46, 30]      # units of up to 16 x 16 items on 4 waves
    with m.Context(0) as own:
        own.set_scene(ar.scene(), hbm=True)
        got = _run(own, ar.params(), ADAPT, rr.RUNS["k jumps by two"][0], _run_name(own, 0, True, (112, 16)), True)
        _equals_replay(got, want, "one block of four waves")


# ---- 8. full stacks ----

def test_full_stacks_with_base_2_grown_to_16(ctx):
    name, cam = "stair32", rf.deep_cameras("stair32")["far"]
    assert dw.DEVICE_DEPTH[name] == 32 == m.MIRT_BVH_MAX_DEPTH
    sd = rf.deep_scene(name, cam)
    ctx.set_scene(sd, hbm=True, bvh="device")
    assert ctx.bvh_info()["plan"]["max_depth"] == 32
    w, h = rf.DEEP_W, rf.DEEP_H
    p = ar.params(spp=2, w=w, h=h, bounces=6)
    case, run = (2, 18, 256), (3, 1 << 30, 16)
    frames = ar.sample_frames(sd, p, 32, name + "far")
    want = rr.replay_run(frames, 2, *case, run)
    assert want["log"][0].tolist() == [w * h, 16] and want["log"][1][1] == 16 and 0 < want["log"][1][0] < w * h and want["log"][2].tolist() == [0, 0]
    after = {}
    for what, (flags, pool) in BUILDS.items():
        q = ar.params(spp=2, w=w, h=h, bounces=6, flags=flags)
        after[what] = _run(ctx, q, case, run, _run_name(ctx, flags, pool, (80, 12)), pool)
        _equals_replay(after[what], want, f"{name}, {what}")
    _same_records(after["pooled"]["records"], after["no grid"]["records"], f"{name}: pooled against MIRT_FLAG_NO_GRID")


# ---- 9. a band and a tile partition ----

@pytest.mark.parametrize("rows", [dict(row_begin=8, row_end=24), dict(row_begin=8, row_end=24, tile_rows=4, n_parts=2, part=1)],
                         ids=["band", "tile partition"])
def test_a_band_keeps_the_absolute_pixels_streams(ctx, rows):
    p = ar.params(**rows)
    n_rows = m.params_out_rows(p)
    assert n_rows == (16 if "tile_rows" not in rows else 8)
    frames = ar.sample_frames(ar.scene(), p, rr.N_FRAMES, "field300")
    run = (4, n_rows * W * 4, 16)                                # the first step stays at 4; shorter lists double
    want = rr.replay_run(frames, rr.BASE, *ADAPT, run)
    log = want["log"].tolist()
    assert log[0] == [n_rows * W, 4] and log[1][1] > 4 and 0 < log[2][0] < log[1][0] < n_rows * W, log
    ctx.set_scene(ar.scene(), hbm=True)
    for pool in (False, True):
        got = _run(ctx, p, ADAPT, run, _run_name(ctx, 0, pool), pool)
        _equals_replay(got, want, f"rows {rows}, pooled {pool}")


# ---- 10. the device form: a run and its resolve on a caller's stream ----

def test_a_run_and_its_resolve_on_a_callers_stream(ctx):
    import torch
    want = rr.reference_run("three sizes")
    ctx.set_scene(ar.scene(), hbm=True)
    p = ar.params()
    stream = torch.cuda.Stream(device="cuda:0")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    ctx.adapt_reset(p)
    torch.cuda.synchronize()
    ctx.adapt_run(p, m.make_adapt_params(*ADAPT, pool=True), m.make_adapt_run(*rr.RUNS["three sizes"][0]), stream=stream.cuda_stream)
    ctx.adapt_resolve_device(p, out.data_ptr(), stream=stream.cuda_stream)      # no host call in between
    assert ctx.last_kernel() == _run_name(ctx, 0, True)
    stream.synchronize()
    img = out.cpu().numpy().reshape(-1, 4)
    recs = want["steps"][-1]["records"]
    assert (img[:, 3] == 255).all()
    for n in np.unique(recs["samples"]):
        sel = recs["samples"] == n
        assert np.array_equal(img[sel, :3], ob.resolve_channel(recs["sum"][sel], int(n), 0)), f"pixels of {n} samples"
    got = _state(ctx)
    got["log"] = ctx.adapt_run_log()
    _equals_replay(got, want, "the device form on a caller's stream")
    assert ctx.adapt_stats()["kernel_ms"] > 0.0


# ---- 11. refusals leave no trace ----

def test_refusals_leave_no_trace(ctx):
    lib = m.lib()
    ctx.set_scene(ar.scene(), hbm=True)
    p, adapt, run = ar.params(), m.make_adapt_params(*ADAPT, pool=True), m.make_adapt_run(3, 3000, 16)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    accum_before, stats_before = ctx.accum_read(p).copy(), ctx.stats()
    ctx.adapt_reset(p)
    n, small = C.c_uint32(77), np.zeros((256, 2), np.uint32)
    assert lib.mirt_ctx_adapt_run_read(ctx._h, C.c_void_p(small.ctypes.data), 256, C.byref(n)) == _abi.MIRT_ERR_NO_SCENE and n.value == 77
    ctx.adapt_step(p, adapt)                                            # a step is no run: still no log
    assert lib.mirt_ctx_adapt_run_read(ctx._h, C.c_void_p(small.ctypes.data), 256, C.byref(n)) == _abi.MIRT_ERR_NO_SCENE
    ctx.adapt_reset(p)
    ctx.adapt_run(p, adapt, run)
    kernel_before = ctx.last_kernel()
    assert kernel_before == _run_name(ctx, 0, True, (112, 16))
    before, list_before, st_before, log_before = ctx.adapt_read(), ctx.adapt_list(), ctx.adapt_stats(), ctx.adapt_run_log()
    assert log_before.tolist() == [[1536, 4], [731, 8], [540, 8]] and len(list_before) == 540

    def refused(params, ad, rn, code, what):
        rc = lib.mirt_ctx_adapt_run_device(ctx._h, C.byref(params) if params is not None else None, C.byref(ad) if ad is not None else None,
                                           C.byref(rn) if rn is not None else None, None)
        assert rc == code, f"{what}: {_abi.STATUS.get(rc, rc)} ({lib.mirt_last_error().decode()})"
        _same_records(ctx.adapt_read(), before, what)
        st = ctx.adapt_stats()
        assert np.array_equal(ctx.adapt_list(), list_before) and (st["steps"], st["total_samples"], st["active"]) == \
            (st_before["steps"], st_before["total_samples"], st_before["active"]), what
        assert np.array_equal(ctx.adapt_run_log(), log_before) and ctx.last_kernel() == kernel_before, what

    def a_run(max_steps=3, min_items=3000, max_spp=16, flags=0):
        r = m.make_adapt_run(max_steps, min_items, max_spp)
        r.flags = flags
        return r

    # the run's own
    refused(p, adapt, None, _abi.MIRT_ERR_NULL_POINTER, "run is null")
    refused(None, adapt, run, _abi.MIRT_ERR_NULL_POINTER, "params is null")
    refused(p, None, run, _abi.MIRT_ERR_NULL_POINTER, "adapt is null")
    for flags in (1, 2, 1 << 31):
        refused(p, adapt, a_run(flags=flags), _abi.MIRT_ERR_BAD_MODE, f"run->flags {flags:#x}")
    for steps in (0, 257, 0xffffffff):
        refused(p, adapt, a_run(max_steps=steps), _abi.MIRT_ERR_BAD_ROWS, f"max_steps {steps}")
    for cap in (2, 6, 12, 24, _abi.MIRT_MAX_SPP_PER_CALL * 2):
        refused(p, adapt, a_run(max_spp=cap), _abi.MIRT_ERR_SPP_RANGE, f"max_spp {cap} with spp 4")
    # a step's, in a step's order: they come before the run's own
    bad_flags = m.make_adapt_params(*ADAPT)
    bad_flags.flags = 1
    refused(p, bad_flags, a_run(flags=1, max_steps=0), _abi.MIRT_ERR_BAD_MODE, "adapt->flags != 0")
    refused(ar.params(spp=3), adapt, a_run(max_steps=0), _abi.MIRT_ERR_SPP_RANGE, "odd spp")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PT, seed=ar.SEED, frame_spp=2), adapt, a_run(max_steps=0), _abi.MIRT_ERR_FRAME_SPP, "frame_spp != 0")
    refused(ar.params(flags=m.MIRT_FLAG_COUNT_WORK), adapt, run, _abi.MIRT_ERR_BAD_MODE, "MIRT_FLAG_COUNT_WORK")
    refused(ar.params(w=W + 1), adapt, a_run(max_steps=0), _abi.MIRT_ERR_OUT_BUFFER, "another width")
    refused(ar.params(row_begin=0, row_end=H - 1), adapt, run, _abi.MIRT_ERR_OUT_BUFFER, "another row count")
    refused(ar.params(spp=0), adapt, run, _abi.MIRT_ERR_SPP_ZERO, "spp == 0")
    refused(ar.params(flags=HOSEK), adapt, run, _abi.MIRT_ERR_SKY, "MIRT_FLAG_SKY_HOSEK without a blob")
    refused(m.make_params(W, H, 4, mode=m.MIRT_MODE_PARITY), adapt, run, _abi.MIRT_ERR_BAD_MODE, "parity mode")
    refused(p, m.make_adapt_params(4, _abi.MIRT_MAX_SPP_PER_CALL + 1, 4096), run, _abi.MIRT_ERR_SPP_RANGE, "max_samples above the per-call limit")
    # runs touched neither the accumulation nor MirtStats
    assert np.array_equal(ctx.accum_read(p), accum_before) and ctx.accum_samples() == 4
    stats_after = ctx.stats()
    assert stats_after["launches"] == 0 and stats_after["samples"] == stats_before["samples"] and stats_after["kernel_ms"] == stats_before["kernel_ms"]
    # no MIRT_SCENE_HBM scene: an LDS scene refuses the run, and a fresh context too
    ctx.set_scene(ar.scene())
    refused(p, adapt, run, _abi.MIRT_ERR_NO_SCENE, "an LDS scene")
    with m.Context(0) as fresh:
        assert lib.mirt_ctx_adapt_run_device(fresh._h, C.byref(p), C.byref(adapt), C.byref(run), None) == _abi.MIRT_ERR_NO_SCENE
        assert lib.mirt_ctx_adapt_run_read(fresh._h, C.c_void_p(small.ctypes.data), 256, C.byref(n)) == _abi.MIRT_ERR_NO_SCENE


# ---- 12. the host object ----

def test_raytracer_render_adaptive_with_a_run():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(W, H), sampling=m.SamplingParams(max_samples_per_pixel=32, num_samples_per_pixel=4, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        c = rt._ctx
        # run=None is today's loop: the steps driven by hand give its image and counts
        img0, counts0 = rt.render_adaptive(4096, 32, seed=3)
        assert c.last_kernel() == "adapt_pixels_kernel<%s,true>" % TF[rt.sky_state is not None]
        flags = HOSEK if rt.sky_state is not None else 0
        p, adapt = m.make_params(W, H, 4, mode=m.MIRT_MODE_PT, num_bounces=8, seed=3, flags=flags), m.make_adapt_params(4, 32, 4096)
        c.adapt_reset(p)
        steps = 0
        while True:
            c.adapt_step(p, adapt)
            steps += 1
            if c.adapt_stats()["active"] == 0:
                break
        assert np.array_equal(c.adapt_resolve(p), img0) and np.array_equal(c.adapt_read()["samples"].reshape(H, W), counts0) and steps > 2
        # a run: the replay's counts, and the oracle's resolve of the replay's sums per count
        run = m.make_adapt_run(9, 3000, 16)
        img, counts = rt.render_adaptive(4096, 32, seed=3, run=run)
        assert c.last_kernel() == _run_name(c, flags, False) and c.adapt_stats()["steps"] == 9
        frames = ar.sample_frames(rt.scene_data(), p, rr.N_FRAMES, "three spheres")
        want = rr.replay_run(frames, 4, 4, 32, 4096, run)
        assert len({int(s) for _, s in want["log"] if s}) >= 2 and want["log"][-1].tolist() == [0, 0], want["log"].tolist()
        assert np.array_equal(c.adapt_run_log(), want["log"])
        recs = want["steps"][-1]["records"]
        _same_records(c.adapt_read(), recs, "render_adaptive(run=...)")
        assert counts.dtype == np.uint32 and np.array_equal(counts, recs["samples"].reshape(H, W)) and c.adapt_stats()["total_samples"] == int(counts.sum())
        flat = img.reshape(-1, 4)
        for n in np.unique(recs["samples"]):
            sel = recs["samples"] == n
            assert np.array_equal(flat[sel, :3], ob.resolve_channel(recs["sum"][sel], int(n), 0)), f"pixels of {n} samples"
        # pooled: the same bytes; run=True: a default run that converges
        img_p, counts_p = rt.render_adaptive(4096, 32, seed=3, run=run, pool=True)
        assert c.last_kernel() == _run_name(c, flags, True) and np.array_equal(img_p, img) and np.array_equal(counts_p, counts)
        img_t, counts_t = rt.render_adaptive(4096, 32, seed=3, run=True, pool=True)
        assert c.last_kernel() == _run_name(c, flags, True) and c.adapt_stats() ["active"] == 0 and c.adapt_stats()["steps"] == 9
        assert counts_t.min() >= 4 and not m.adapt_active(c.adapt_read(), adapt).any() and c.adapt_run_log()[-1].tolist() == [0, 0]
        with pytest.raises(ValueError):
            rt.render_adaptive(4096, 32, run=(9, 3000, 16))
    finally:
        rt.close()
