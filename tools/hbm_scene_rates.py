#!/usr/bin/env python3
"""MIRT_SCENE_HBM rates: one JSON line per case.

  rtiow    RTIOW (484 spheres) at 1080p x 2 / 16 / 128 spp: the default LDS build against the HBM build (BVH in device memory), same
           process, interleaved rounds, median kernel time of --reps launches after a warm-up
  field    RTIOW-style fields of 10 k / 100 k / 1 M spheres at 1080p x 16 spp (HBM only): Msamples/s, kernel ms, the time of
           mirt_ctx_set_scene_ex (host BVH build + upload), the mirt_bvh_plan statistics, and sphere tests / BVH nodes per ray from a
           counting launch (MIRT_FLAG_COUNT_WORK | MIRT_FLAG_COUNT_GRID) at 480x270 x 2 spp

usage: python tools/hbm_scene_rates.py [--reps 5] [--fields 10000,100000,1000000]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import c_spheres, look, rtiow_field, scene_from_arrays   # noqa: E402
from helpers import scene_data                             # noqa: E402

W, H = 1920, 1080


def kernel_ms(ctx, p) -> float:
    ctx.render(p)
    return ctx.stats()["kernel_ms"]


def rtiow_cases(reps: int):
    sd = scene_data("rtiow_final", W, H)
    ctx_lds, ctx_hbm = m.Context(0), m.Context(0)
    ctx_lds.set_scene(sd)
    ctx_hbm.set_scene(sd, hbm=True)
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
        print(json.dumps({"case": "rtiow", "spp": spp, "width": W, "height": H, "lds_ms": round(lds, 3), "hbm_ms": round(hbm, 3),
                          "hbm_over_lds": round(hbm / lds, 3), "lds_kernel": k_lds, "hbm_kernel": ctx_hbm.last_kernel(),
                          "lds_all_ms": [round(x, 3) for x in t["lds"]], "hbm_all_ms": [round(x, 3) for x in t["hbm"]]}), flush=True)
    ctx_lds.close()
    ctx_hbm.close()


def field_case(n: int, reps: int):
    arr, mats, tex = rtiow_field(n, seed=n)
    carr, keep = c_spheres(arr)
    plan = m.bvh_plan(carr)
    ctx = m.Context(0)
    sd = scene_from_arrays(look(W, H, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    t0 = time.perf_counter()
    ctx.set_scene(sd, hbm=True)
    build_ms = (time.perf_counter() - t0) * 1e3
    spp = 16
    p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
    kernel_ms(ctx, p)
    ts = [kernel_ms(ctx, p) for _ in range(reps)]
    ms = statistics.median(ts)
    # work per ray from a counting launch of the BVH build (a smaller frame: the counting build runs lane = sample)
    sdc = scene_from_arrays(look(480, 270, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    ctx.set_scene(sdc, hbm=True)
    ctx.render(m.make_params(480, 270, 2, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID))
    st = ctx.stats()
    print(json.dumps({"case": "field", "n_spheres": n, "spp": spp, "width": W, "height": H, "kernel_ms": round(ms, 3),
                      "all_ms": [round(x, 3) for x in ts], "msamples_per_s": round(W * H * spp / ms / 1e3, 1),
                      "set_scene_ex_ms": round(build_ms, 1), "plan": plan,
                      "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["grid_cells"] / st["rays"], 2),
                      "kernel": "render_pt_hbm_kernel<false,false,true,true>"}), flush=True)
    ctx.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", default="10000,100000,1000000")
    ap.add_argument("--skip-rtiow", action="store_true")
    a = ap.parse_args()
    if not a.skip_rtiow:
        rtiow_cases(a.reps)
    for n in (int(x) for x in a.fields.split(",") if x):
        field_case(n, a.reps)


if __name__ == "__main__":
    main()
