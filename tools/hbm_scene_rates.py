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

usage: python tools/hbm_scene_rates.py [--reps 5] [--fields 10000,100000,1000000] [--bvh host|device|both] [--soup 100000]
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


def _timed_set_scene(ctx, sd, bvh: str):
    """-> (wall ms of the set_scene call, the device build's parts as the library reports them on stderr, or {})."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            ctx.set_scene(sd, hbm=True, bvh=bvh)
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    parts = {k: float(v) for k, v in re.findall(r"(always_ms|upload_ms|kernels_ms)=([0-9.]+)", text)}
    return wall, parts


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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", default="10000,100000,1000000")
    ap.add_argument("--skip-rtiow", action="store_true")
    ap.add_argument("--bvh", choices=("host", "device", "both"), default="host")
    ap.add_argument("--soup", type=int, default=100000, help="--bvh both: spheres of the clustered soup (0: none)")
    a = ap.parse_args()
    fields = [int(x) for x in a.fields.split(",") if x]
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
