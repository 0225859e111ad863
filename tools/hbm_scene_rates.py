#!/usr/bin/env python3
"""MIRT_SCENE_HBM rates: one JSON line per case.

  rtiow    RTIOW (484 spheres) at 1080p x 2 / 16 / 128 spp: the default LDS build against the HBM build (BVH in device memory), same
           process, interleaved rounds, median kernel time of --reps launches after a warm-up
  field    RTIOW-style fields of 10 k / 100 k / 1 M spheres at 1080p x 16 spp (HBM only): Msamples/s, kernel ms, the time of
           mirt_ctx_set_scene_ex (host BVH build + upload), the mirt_bvh_plan statistics, and sphere tests / BVH nodes per ray from a
           counting launch (MIRT_FLAG_COUNT_WORK | MIRT_FLAG_COUNT_GRID) at 480x270 x 2 spp

  builders (--bvh both) the host builder against the device builder (MIRT_SCENE_BVH_DEVICE) on the same fields and on
           clustered_soup(--soup): one process, the two alternating, median of --reps mirt_ctx_set_scene_ex calls after a warm-up; the
           device build's parts (the host's always-list pass, the uploads, the build kernels between two events: the library reports
           them on stderr when MIRT_BVH_TIMING is set); n_nodes / max_depth; tests and nodes per ray; kernel ms at 1080p x 16 spp
  --bvh host (default) / device: the rtiow and field cases with that builder

  --update in-place updates (mirt_ctx_update_spheres / _device) on the same fields, device-built tree: one process, alternating with
           the mirt_ctx_set_scene_ex(HBM | BVH_DEVICE) of the same moved world that they replace; median of --reps after a warm-up; the
           update's parts between events (scatter, refit levels, bounds: MIRT_BVH_TIMING); then kernel ms at 1080p x 16 spp and tests /
           nodes per ray after every small sphere moved by up to 0.25, 1 and 4 median radii in x and z -- the refitted tree against
           a fresh device tree and a fresh host tree of the same world: after how much motion a rebuild pays

  --set-spheres a whole new sphere table for a resident scene (mirt_ctx_set_spheres / _device) on the same fields, one process per
           field (give one --fields value per run): the three routes to a device-built tree of the same world, alternating on two
           contexts -- (a) mirt_ctx_set_scene_ex(HBM | BVH_DEVICE) from host memory, (b) mirt_ctx_set_spheres from host memory,
           (c) mirt_ctx_set_spheres_device from a torch buffer; wall time, median of --reps after a warm-up; the parts the library
           reports (MIRT_BVH_TIMING): (a) always list, upload, build kernels; (b), (c) census, always list, prepare, build kernels

  --pool   the pooled schedule (MIRT_FLAG_KERNEL_POOL on an HBM scene: render_pt_pool_hbm_kernel) against the default
           strip kernel on the worlds of DESIGN.md 10.2: RTIOW at 1080p x 2 / 16 / 128 spp, the 10 k / 100 k / 1 M fields at 16 and
           128 spp.  One child process per world, each under its own time limit (--step-timeout), the next one only after the last
           has ended well; inside a child both kernels run on one context in alternating windows -- a window is as many launches as
           add up to --window-ms of kernel time, its figure their mean -- and the median of --reps windows after a warm-up window of
           each is reported, with the images compared once.  MIRT_HBM_POOL_SLOTS / MIRT_POOL_BLOCKS_PER_CU (A/B runs of the geometry)
           pass through to the children and are recorded.  --pool-counts adds the lane use of both schedules from counting launches
           (480x270 x 32 spp): traversal = grid_cells / (64 grid_wave_cells), step = lane_iterations / (64 wave_iterations).

usage: python tools/hbm_scene_rates.py [--reps 5] [--fields 10000,100000,1000000] [--bvh host|device|both] [--soup 100000] [--update | --set-spheres | --pool]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import c_spheres, clustered_soup, look, rtiow_field, scene_from_arrays   # noqa: E402
from helpers import scene_data                             # noqa: E402

W, H = 1920, 1080


def kernel_ms(ctx, p) -> float:
    ctx.render(p)
    return ctx.stats()["kernel_ms"]


def rtiow_cases(reps: int, bvh: str = "host"):
    sd = scene_data("rtiow_final", W, H)
    ctx_lds, ctx_hbm = m.Context(0), m.Context(0)
    ctx_lds.set_scene(sd)
    ctx_hbm.set_scene(sd, hbm=True, bvh=bvh)
    for spp in (2, 16, 128):
        p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
        kernel_ms(ctx_lds, p), kernel_ms(ctx_hbm, p)             # warm-up
        t = {"lds": [], "hbm": []}
        for _ in range(reps):                                      # interleaved rounds
            t["lds"].append(kernel_ms(ctx_lds, p))
            t["hbm"].append(kernel_ms(ctx_hbm, p))
        lds, hbm = statistics.median(t["lds"]), statistics.median(t["hbm"])
        ctx_lds.render(p)
        k_lds = ctx_lds.last_kernel()
        ctx_hbm.render(p)
        print(json.dumps({"case": "rtiow", "bvh": bvh, "spp": spp, "width": W, "height": H, "lds_ms": round(lds, 3), "hbm_ms": round(hbm, 3),
                          "hbm_over_lds": round(hbm / lds, 3), "lds_kernel": k_lds, "hbm_kernel": ctx_hbm.last_kernel(),
                          "lds_all_ms": [round(x, 3) for x in t["lds"]], "hbm_all_ms": [round(x, 3) for x in t["hbm"]]}), flush=True)
    ctx_lds.close()
    ctx_hbm.close()


def field_case(n: int, reps: int, bvh: str = "host"):
    arr, mats, tex = rtiow_field(n, seed=n)
    ctx = m.Context(0)
    sd = scene_from_arrays(look(W, H, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    t0 = time.perf_counter()
    ctx.set_scene(sd, hbm=True, bvh=bvh)
    build_ms = (time.perf_counter() - t0) * 1e3
    plan = ctx.bvh_info()["plan"]
    spp = 16
    p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
    kernel_ms(ctx, p)
    ts = [kernel_ms(ctx, p) for _ in range(reps)]
    ms = statistics.median(ts)
    # work per ray from a counting launch of the BVH build (a smaller frame: the counting build runs lane = sample)
    sdc = scene_from_arrays(look(480, 270, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    ctx.set_scene(sdc, hbm=True, bvh=bvh)
    ctx.render(m.make_params(480, 270, 2, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID))
    st = ctx.stats()
    print(json.dumps({"case": "field", "bvh": bvh, "n_spheres": n, "spp": spp, "width": W, "height": H, "kernel_ms": round(ms, 3),
                      "all_ms": [round(x, 3) for x in ts], "msamples_per_s": round(W * H * spp / ms / 1e3, 1),
                      "set_scene_ex_ms": round(build_ms, 1), "plan": plan,
                      "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["grid_cells"] / st["rays"], 2),
                      "kernel": "render_pt_hbm_kernel<false,false,true,true>"}), flush=True)
    ctx.close()


def _timed_stderr(fn, pattern):
    """-> (wall ms of fn(), {key: value} the library reported on stderr meanwhile)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return wall, {k: float(v) for k, v in re.findall(pattern, text)}


def _timed_set_scene(ctx, sd, bvh: str):
    """-> (wall ms of the set_scene call, the device build's parts as the library reports them on stderr, or {})."""
    return _timed_stderr(lambda: ctx.set_scene(sd, hbm=True, bvh=bvh), r"(always_ms|upload_ms|kernels_ms)=([0-9.]+)")


def builders_case(name: str, arr, mats, tex, eye, reps: int):
    os.environ["MIRT_BVH_TIMING"] = "1"
    med = statistics.median
    sd = scene_from_arrays(look(W, H, eye, (0, 0, 0), vfov=35), arr, mats, tex)
    sdc = scene_from_arrays(look(480, 270, eye, (0, 0, 0), vfov=35), arr, mats, tex)
    ctxs = {"host": m.Context(0), "device": m.Context(0)}
    wall = {"host": [], "device": []}
    parts = {"always_ms": [], "upload_ms": [], "kernels_ms": []}
    for rnd in range(reps + 1):                                     # round 0 = warm-up (allocations, code objects)
        for b in ("host", "device"):
            w, pt = _timed_set_scene(ctxs[b], sd, b)
            if rnd:
                wall[b].append(w)
                for k in parts:
                    if k in pt:
                        parts[k].append(pt[k])
    p = m.make_params(W, H, 16, mode=m.MIRT_MODE_PT, num_bounces=8)
    render = {"host": [], "device": []}
    for rnd in range(reps + 1):
        for b in ("host", "device"):
            t = kernel_ms(ctxs[b], p)
            if rnd:
                render[b].append(t)
    out = {"case": "builders", "world": name, "n_spheres": int(len(arr)), "reps": reps, "width": W, "height": H, "spp": 16}
    for b in ("host", "device"):
        plan = ctxs[b].bvh_info()["plan"]
        ctxs[b].set_scene(sdc, hbm=True, bvh=b)
        ctxs[b].render(m.make_params(480, 270, 2, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID))
        st = ctxs[b].stats()
        out[b] = {"set_scene_ex_ms": round(med(wall[b]), 2), "set_scene_ex_all_ms": [round(x, 2) for x in wall[b]],
                  "n_nodes": plan["n_nodes"], "max_depth": plan["max_depth"], "n_always": plan["n_always"],
                  "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["grid_cells"] / st["rays"], 2),
                  "render_ms": round(med(render[b]), 3), "render_all_ms": [round(x, 3) for x in render[b]]}
        ctxs[b].close()
    out["device"].update({k: round(med(v), 3) for k, v in parts.items() if v})
    out["render_device_over_host"] = round(out["device"]["render_ms"] / out["host"]["render_ms"], 3)
    out["set_scene_host_over_device"] = round(out["host"]["set_scene_ex_ms"] / out["device"]["set_scene_ex_ms"], 2)
    print(json.dumps(out), flush=True)


def _jittered(arr, radii: float, seed: int):
    """Every small sphere of an rtiow_field moved by up to `radii` median radii in x and z."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = arr.copy()
    step = radii * float(np.median(arr["radius"][5:]))
    out["center"][5:, 0] += rng.uniform(-step, step, len(arr) - 5).astype(np.float32)
    out["center"][5:, 2] += rng.uniform(-step, step, len(arr) - 5).astype(np.float32)
    return out


def update_case(n: int, reps: int):
    import numpy as np
    import torch
    os.environ["MIRT_BVH_TIMING"] = "1"
    med = statistics.median
    arr, mats, tex = rtiow_field(n, seed=n)
    eye = (40, 6, 30)
    cam, cam_count = look(W, H, eye, (0, 0, 0), vfov=35), look(480, 270, eye, (0, 0, 0), vfov=35)
    worlds = [_jittered(arr, 0.25, 1), _jittered(arr, 0.25, 2)]
    scenes = [scene_from_arrays(cam, w, mats, tex) for w in worlds]
    d_worlds = [torch.from_numpy(w.view(np.uint8).copy()).to("cuda:0") for w in worlds]
    ctx, ctx_rebuild = m.Context(0), m.Context(0)
    ctx.set_scene(scene_from_arrays(cam, arr, mats, tex), hbm=True, bvh="device")
    refit_pat, build_pat = r"(scatter_ms|refit_ms|bounds_ms|levels)=([0-9.]+)", r"(always_ms|upload_ms|kernels_ms)=([0-9.]+)"
    wall = {"update_spheres": [], "update_spheres_device": [], "rebuild": []}
    parts = {}
    for rnd in range(reps + 1):                                     # round 0 = warm-up (the refit's schedule, allocations, code objects)
        k = rnd & 1
        t_host, p_host = _timed_stderr(lambda: ctx.update_spheres(0, worlds[k]), refit_pat)
        t_dev, p_dev = _timed_stderr(lambda: ctx.update_spheres_device(0, n, d_worlds[1 - k].data_ptr()), refit_pat)
        t_build, p_build = _timed_stderr(lambda: ctx_rebuild.set_scene(scenes[k], hbm=True, bvh="device"), build_pat)
        if rnd:
            wall["update_spheres"].append(t_host)
            wall["update_spheres_device"].append(t_dev)
            wall["rebuild"].append(t_build)
            for src, pt in (("host", p_host), ("device", p_dev), ("rebuild", p_build)):
                for key, v in pt.items():
                    parts.setdefault(f"{src}_{key}", []).append(v)
    out = {"case": "update", "world": f"rtiow_field({n})", "n_spheres": n, "reps": reps, "n_nodes": ctx.bvh_info()["plan"]["n_nodes"],
           "refits": ctx.bvh_refits()}
    for k, v in wall.items():
        out[f"{k}_ms"] = round(med(v), 3)
        out[f"{k}_all_ms"] = [round(x, 3) for x in v]
    out.update({k: round(med(v), 3) for k, v in parts.items()})
    out["rebuild_over_update"] = round(out["rebuild_ms"] / out["update_spheres_ms"], 2)
    out["rebuild_over_update_device"] = round(out["rebuild_ms"] / out["update_spheres_device_ms"], 2)
    print(json.dumps(out), flush=True)

    # how much worse a refitted tree culls, and renders, than a fresh one of the same world
    p = m.make_params(W, H, 16, mode=m.MIRT_MODE_PT, num_bounces=8)
    pc = m.make_params(480, 270, 2, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID)
    for radii in (0.25, 1.0, 4.0):
        moved = _jittered(arr, radii, 3)
        sd = scene_from_arrays(cam, moved, mats, tex)
        row = {"case": "update_culling", "world": f"rtiow_field({n})", "n_spheres": n, "jitter_median_radii": radii, "spp": 16, "width": W, "height": H}
        for name in ("refitted", "fresh_device", "fresh_host"):
            if name == "refitted":
                ctx.set_scene(scene_from_arrays(cam, arr, mats, tex), hbm=True, bvh="device")
                ctx.update_spheres(0, moved)
            else:
                ctx.set_scene(sd, hbm=True, bvh="device" if name == "fresh_device" else "host")
            kernel_ms(ctx, p)
            ts = [kernel_ms(ctx, p) for _ in range(reps)]
            ctx.set_camera(cam_count)
            ctx.render(pc)
            st = ctx.stats()
            row[name] = {"render_ms": round(med(ts), 3), "render_all_ms": [round(x, 3) for x in ts],
                         "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["grid_cells"] / st["rays"], 2)}
        row["render_refitted_over_fresh_host"] = round(row["refitted"]["render_ms"] / row["fresh_host"]["render_ms"], 3)
        row["render_refitted_over_fresh_device"] = round(row["refitted"]["render_ms"] / row["fresh_device"]["render_ms"], 3)
        row["tests_refitted_over_fresh_host"] = round(row["refitted"]["tests_per_ray"] / row["fresh_host"]["tests_per_ray"], 3)
        print(json.dumps(row), flush=True)
    ctx.close()
    ctx_rebuild.close()


def set_spheres_case(n: int, reps: int):
    import numpy as np
    import torch
    os.environ["MIRT_BVH_TIMING"] = "1"
    med = statistics.median
    arr, mats, tex = rtiow_field(n, seed=n)
    cam = look(W, H, (40, 6, 30), (0, 0, 0), vfov=35)
    worlds = [_jittered(arr, 0.25, 1), _jittered(arr, 0.25, 2)]        # two worlds in turn: no call finds its own result in place
    scenes = [scene_from_arrays(cam, w, mats, tex) for w in worlds]
    d_worlds = [torch.from_numpy(w.view(np.uint8).copy()).to("cuda:0") for w in worlds]
    ctx, ctx_rebuild = m.Context(0), m.Context(0)
    ctx.set_scene(scene_from_arrays(cam, arr, mats, tex), hbm=True, bvh="device")
    set_pat, build_pat = r"(census_ms|always_ms|prepare_ms|kernels_ms)=([0-9.]+)", r"(always_ms|upload_ms|kernels_ms)=([0-9.]+)"
    wall = {"set_scene_ex": [], "set_spheres": [], "set_spheres_device": []}
    parts = {}
    for rnd in range(reps + 1):                                     # round 0 = warm-up (allocations, code objects)
        k = rnd & 1
        t_build, p_build = _timed_stderr(lambda: ctx_rebuild.set_scene(scenes[k], hbm=True, bvh="device"), build_pat)
        t_host, p_host = _timed_stderr(lambda: ctx.set_spheres(worlds[k]), set_pat)
        t_dev, p_dev = _timed_stderr(lambda: ctx.set_spheres_device(n, d_worlds[1 - k].data_ptr()), set_pat)
        if rnd:
            wall["set_scene_ex"].append(t_build)
            wall["set_spheres"].append(t_host)
            wall["set_spheres_device"].append(t_dev)
            for src, pt in (("set_scene_ex", p_build), ("set_spheres", p_host), ("set_spheres_device", p_dev)):
                for key, v in pt.items():
                    parts.setdefault(f"{src}_{key}", []).append(v)
    ctx.set_spheres(worlds[0])                                      # the three routes end in the same tree
    ctx_rebuild.set_scene(scenes[0], hbm=True, bvh="device")
    same = all(np.array_equal(x, y) for x, y in zip(ctx.bvh_read(), ctx_rebuild.bvh_read()))
    plan = ctx.bvh_info()["plan"]
    out = {"case": "set_spheres", "world": f"rtiow_field({n})", "n_spheres": n, "reps": reps, "n_nodes": plan["n_nodes"], "n_always": plan["n_always"],
           "same_tree_bytes": bool(same)}
    for k, v in wall.items():
        out[f"{k}_ms"] = round(med(v), 3)
        out[f"{k}_all_ms"] = [round(x, 3) for x in v]
    out.update({k: round(med(v), 3) for k, v in parts.items()})
    out["set_spheres_over_set_scene_ex"] = round(out["set_spheres_ms"] / out["set_scene_ex_ms"], 3)
    out["set_spheres_device_over_set_scene_ex"] = round(out["set_spheres_device_ms"] / out["set_scene_ex_ms"], 3)
    print(json.dumps(out), flush=True)
    ctx.close()
    ctx_rebuild.close()


def _window_ms(ctx, p, window_ms: float) -> tuple:
    """One timing window: launches until their kernel times add up to window_ms -> (mean kernel ms, launches)."""
    total, n = 0.0, 0
    while n == 0 or total < window_ms:
        total += kernel_ms(ctx, p)
        n += 1
    return total / n, n


def pool_world(world: str, reps: int, window_ms: float, bvh: str, counts: bool):
    """One world of --pool, in this process: strip and pooled kernel on ONE context, alternating windows."""
    import numpy as np
    if world == "rtiow":
        sd, spps, name = scene_data("rtiow_final", W, H), (2, 16, 128), "rtiow"
        sdc = scene_data("rtiow_final", 480, 270)
    else:
        n = int(world)
        arr, mats, tex = rtiow_field(n, seed=n)
        sd, spps, name = scene_from_arrays(look(W, H, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex), (16, 128), f"rtiow_field({n})"
        sdc = scene_from_arrays(look(480, 270, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    ctx = m.Context(0)
    ctx.set_scene(sd, hbm=True, bvh=bvh)
    depth = ctx.bvh_info()["plan"]["max_depth"]
    knobs = {k: os.environ[k] for k in ("MIRT_HBM_POOL_SLOTS", "MIRT_POOL_BLOCKS_PER_CU") if k in os.environ}
    for spp in spps:
        ps = {"strip": m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8),
              "pool": m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_KERNEL_POOL)}
        imgs, kernels = {}, {}
        for k, p in ps.items():                                     # warm-up: one window of each, and the images compared once
            imgs[k] = ctx.render(p)
            kernels[k] = ctx.last_kernel()
            _window_ms(ctx, p, window_ms)
        t, launches = {"strip": [], "pool": []}, 0
        for _ in range(reps):                                       # alternating windows
            for k, p in ps.items():
                ms, launches = _window_ms(ctx, p, window_ms)
                t[k].append(ms)
        strip, pool = statistics.median(t["strip"]), statistics.median(t["pool"])
        print(json.dumps({"case": "pool", "world": name, "bvh": bvh, "max_depth": depth, "spp": spp, "width": W, "height": H, "strip_ms": round(strip, 3),
                          "pool_ms": round(pool, 3), "pool_over_strip": round(pool / strip, 3), "images_equal": bool(np.array_equal(imgs["strip"], imgs["pool"])),
                          "strip_kernel": kernels["strip"], "pool_kernel": kernels["pool"], "plan": m.bvh_pool_plan(depth), "knobs": knobs,
                          "window_ms": window_ms, "launches_in_last_window": launches,
                          "strip_all_ms": [round(x, 3) for x in t["strip"]], "pool_all_ms": [round(x, 3) for x in t["pool"]]}), flush=True)
    if counts:                                                      # deterministic: no timer
        ctx.set_scene(sdc, hbm=True, bvh=bvh)
        row = {"case": "pool_lane_use", "world": name, "bvh": bvh, "width": 480, "height": 270, "spp": 32}
        count = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID
        for k, flags in (("strip", count), ("pool", count | m.MIRT_FLAG_KERNEL_POOL)):
            ctx.render(m.make_params(480, 270, 32, mode=m.MIRT_MODE_PT, num_bounces=8, flags=flags))
            st = ctx.stats()
            row[k] = {"kernel": ctx.last_kernel(), "traversal_lane_use": round(st["grid_cells"] / (64.0 * st["grid_wave_cells"]), 4),
                      "step_lane_use": round(st["lane_iterations"] / (64.0 * st["wave_iterations"]), 4), "rays": st["rays"],
                      "grid_cells": st["grid_cells"], "grid_wave_cells": st["grid_wave_cells"], "lane_iterations": st["lane_iterations"],
                      "wave_iterations": st["wave_iterations"]}
        print(json.dumps(row), flush=True)
    ctx.close()


def pool_cases(a, fields) -> int:
    """--pool: one child per world under its own time limit; nothing more is started after a child that did not end well."""
    import subprocess
    worlds = ([] if a.skip_rtiow else ["rtiow"]) + [str(n) for n in fields]
    for world in worlds:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--pool-world", world, "--reps", str(a.reps), "--window-ms", str(a.window_ms),
               "--bvh", a.bvh] + (["--pool-counts"] if a.pool_counts else [])
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"case": "pool", "world": world, "error": f"child ended with status {rc}; nothing further was run"}), flush=True)
            return rc
    return 0


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", default="10000,100000,1000000")
    ap.add_argument("--skip-rtiow", action="store_true")
    ap.add_argument("--bvh", choices=("host", "device", "both"), default="host")
    ap.add_argument("--soup", type=int, default=100000, help="--bvh both: spheres of the clustered soup (0: none)")
    ap.add_argument("--update", action="store_true", help="in-place updates against the device rebuild they replace")
    ap.add_argument("--set-spheres", action="store_true", help="a new sphere table by set_spheres / set_spheres_device against set_scene_ex")
    ap.add_argument("--pool", action="store_true", help="the pooled schedule of HBM scenes against the strip kernel, one child process per world")
    ap.add_argument("--pool-counts", action="store_true", help="--pool: also the lane use of both schedules from counting launches")
    ap.add_argument("--pool-world", default="", help=argparse.SUPPRESS)          # a child of --pool: rtiow, or a field's sphere count
    ap.add_argument("--window-ms", type=float, default=100.0, help="--pool: kernel time of one timing window")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="--pool: seconds a world's child process may take")
    a = ap.parse_args()
    fields = [int(x) for x in a.fields.split(",") if x]
    if a.pool_world:
        pool_world(a.pool_world, a.reps, a.window_ms, "host" if a.bvh == "both" else a.bvh, a.pool_counts)
        return
    if a.pool:
        a.bvh = "host" if a.bvh == "both" else a.bvh
        sys.exit(pool_cases(a, fields))
    if a.set_spheres:
        for n in fields:
            set_spheres_case(n, a.reps)
        return
    if a.update:
        for n in fields:
            update_case(n, a.reps)
        return
    if a.bvh == "both":
        for n in fields:
            arr, mats, tex = rtiow_field(n, seed=n)
            builders_case(f"rtiow_field({n})", arr, mats, tex, (40, 6, 30), a.reps)
        if a.soup:
            arr, mats, tex = clustered_soup(a.soup)
            builders_case(f"clustered_soup({a.soup})", arr, mats, tex, (0, 5, 60), a.reps)
        return
    if not a.skip_rtiow:
        rtiow_cases(a.reps, a.bvh)
    for n in fields:
        field_case(n, a.reps, a.bvh)


if __name__ == "__main__":
    main()
