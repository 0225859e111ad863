"""The LDS grid builds where ROUNDING decides a hit (scenes: tests/grid_rounding.py; that they are not vacuous:
test_grid_rounding_cpu.py).

For every scene, every grid build gives the oracle's exact 64-bit sums -- and the sums of the same context's flat scan
(MIRT_FLAG_NO_GRID) --, and every tuning knob of the grid gives the default context's bytes.  Each build is asserted by
last_kernel(), so a changed default cannot silently drop one.  The comparison is exact; a failure names scene, build, knob and the
number of pixels that differ."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
import grid_rounding as gr

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
POOL, STRIP = m.MIRT_FLAG_KERNEL_POOL, m.MIRT_FLAG_KERNEL_STRIP
COUNTING = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID

# build name -> (flags, spp, frame_spp)
BUILDS = {
    "pool 24 spp": (POOL, 24, 0),
    "pool 64 spp": (POOL, 64, 0),
    "strip lane=pixel 3 spp (camera rays through the grid)": (STRIP, 3, 0),
    "strip lane=pixel 8 spp (camera rays through candidate lists)": (STRIP, 8, 0),
    "strip lane=sample 64 spp": (STRIP, 64, 0),
    "frame stream frame_spp=2": (0, 8, 2),
    "default 16 spp": (0, 16, 0),
}
KNOBS = [("MIRT_STRIP_CAND", "0"), ("MIRT_GRID_FLAT_Y", "0"), ("MIRT_GRID_CELL", "1"), ("MIRT_GRID_CELL", "4"), ("MIRT_GRID_CELL", "16"),
         ("MIRT_GRID_BIG", "1"), ("MIRT_GRID_BIG", "64"), ("MIRT_POOL_GRID", "0")]
KNOB_BUILDS = ["pool 24 spp", "strip lane=pixel 3 spp (camera rays through the grid)",
               "strip lane=pixel 8 spp (camera rays through candidate lists)", "strip lane=sample 64 spp", "default 16 spp"]


@pytest.fixture(scope="module")
def contexts():
    """The default context and one per knob value: tuning knobs are read once, in mirt_ctx_create."""
    mp = pytest.MonkeyPatch()
    made = {"default": m.Context(0)}
    try:
        for name, value in KNOBS:
            mp.setenv(name, value)
            made[f"{name}={value}"] = m.Context(0)
            mp.delenv(name)
        yield made
    finally:
        mp.undo()
        for c in made.values():
            c.close()


def _bounces(scene):
    return 6 if scene == "far origins" else 4


def _params(scene, w, h, build, extra_flags=0):
    flags, spp, frame_spp = BUILDS[build]
    return m.make_params(w, h, spp, mode=PT, num_bounces=_bounces(scene), flags=flags | extra_flags, frame_spp=frame_spp)


def _sums(ctx, p):
    ctx.accum_reset(p)
    ctx.accum_add(p)
    return ctx.accum_read(p)


def _differ(a, b):
    return int((a != b).any(axis=-1).sum())


def _check_kernel(name, build, has_grid, flat_y, knob=None):
    """The build that ran, by name: render_pt_pool_kernel<1024, SLOTS, ..., COUNT, HOSEK, 1, GRID, FLATY>,
    render_pt_strip[_frame]_kernel<COUNT, HOSEK, GRID, lane = pixel>."""
    name = name.replace("_frame_kernel", "_kernel")
    fy = "true" if flat_y else "false"
    if not has_grid:
        assert not name.endswith(",1,true,true>") and not name.endswith(",1,true,false>") and "render_pt_strip_kernel<false,false,true," not in name, (build, name)
        return
    pool_grid = name.startswith("render_pt_pool_kernel<1024,") and name.endswith(f",1,true,{fy}>")
    if build.startswith("pool"):
        assert pool_grid, (build, name)
    elif build.startswith("strip lane=pixel") or build.startswith("frame stream") or build.startswith("progressive"):
        assert name == "render_pt_strip_kernel<false,false,true,true>", (build, name)
    elif build.startswith("strip lane=sample"):
        assert name == "render_pt_strip_kernel<false,false,true,false>", (build, name)
    else:
        assert pool_grid or name.startswith("render_pt_strip_kernel<false,false,true,"), (build, name)


@pytest.mark.parametrize("scene", list(gr.SCENES))
def test_grid_builds_are_exact_where_rounding_decides(contexts, oracle, scene):
    build, has_grid = gr.SCENES[scene]
    sd, w, h = build()
    plan = gr.grid_plan(sd)
    cen, rad = gr.spheres_of(sd)
    flat_y = has_grid and int(gr.binning(cen, rad, plan.cell_factor)["dims"][1]) == 1
    ctx = contexts["default"]
    for c in contexts.values():
        c.set_scene(sd)
    failures, default_sums = [], {}

    def compare(got, want, build_name, knob, against):
        n = _differ(got, want)
        print(f"{scene} | {build_name} | {knob} | against {against}: {n} of {w * h} pixels differ")
        if n:
            failures.append(f"{scene} | {build_name} | {knob} | against {against}: {n} of {w * h} pixels differ")

    # every build of the default context: the oracle's sums, and the same context's flat scan
    for name in BUILDS:
        p = _params(scene, w, h, name)
        got = _sums(ctx, p)
        _check_kernel(ctx.last_kernel(), name, has_grid, flat_y)
        default_sums[name] = got
        compare(got, oracle.render_pt_sums(sd, p), name, "default", "the oracle")
        try:
            flat = _sums(ctx, _params(scene, w, h, name, m.MIRT_FLAG_NO_GRID))
        except m.MirtError as e:                                     # the flat kernel does not fit beside this scene's tables
            assert e.status_name == "MIRT_ERR_SCENE_TOO_LARGE", e
        else:
            _check_kernel(ctx.last_kernel(), name, False, False)     # a flat scan, whatever the scene
            compare(got, flat, name, "default", "MIRT_FLAG_NO_GRID")

    # the pooled grid build's counting build: the paths are the flat scan's, ray by ray
    p = _params(scene, w, h, "pool 24 spp")
    want_img = oracle.render(sd, _params(scene, w, h, "pool 24 spp", m.MIRT_FLAG_COUNT_WORK))
    want_counts = oracle.stats()
    got_img = ctx.render(_params(scene, w, h, "pool 24 spp", COUNTING))
    kname, st = ctx.last_kernel(), ctx.stats()
    if has_grid and plan.pool_slots in (160, 152):                  # (counting builds of the grid kernel exist for its two largest pool geometries)
        _check_kernel(kname, "pool counting", True, flat_y)
        assert ",true,false,1," in kname, kname
    compare(got_img, want_img, "pool counting build (image)", "default", "the oracle")
    for k in ("rays", "hits", "sky_misses", "scatter"):
        if st[k] != want_counts[k]:
            failures.append(f"{scene} | pool counting build | default | counter {k}: {st[k]} against the oracle's {want_counts[k]}")

    # one progressive frame in one launch (the frame builds)
    import torch
    pf = m.make_params(w, h, 4, mode=PT, num_bounces=_bounces(scene))
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.accum_reset(pf)
    ctx.accum_frame_device(pf, out.data_ptr())
    ctx.synchronize()
    assert "_frame_kernel<" in ctx.last_kernel(), ctx.last_kernel()
    _check_kernel(ctx.last_kernel(), "progressive frame", has_grid, flat_y)
    compare(ctx.accum_read(pf), oracle.render_pt_sums(sd, pf), "progressive frame (sums)", "default", "the oracle")
    compare(out.cpu().numpy(), oracle.render(sd, pf), "progressive frame (image)", "default", "the oracle")

    # every knob: the default context's bytes
    for knob, c in contexts.items():
        if knob == "default":
            continue
        for name in KNOB_BUILDS:
            compare(_sums(c, _params(scene, w, h, name)), default_sums[name], name, knob, "the default context")
    assert not failures, "\n".join([f"{len(failures)} comparisons differ:"] + failures)
