#!/usr/bin/env python3
"""Ray-query rates (mirt_ctx_trace_rays_device): one JSON line per case.

The rays are the 1920 x 1080 pixel-centre rays of the camera of DESIGN.md 10.2 on the RTIOW-style fields of 10 k / 100 k / 1 M spheres
(tools/hbm_scene_rates.py's worlds), in image order and -- the same rays -- shuffled: what incoherence costs a lane-per-ray schedule
that does not sort.  Per field and order: nearest hit and any hit through the tree, and for the 10 k field the flat scan; kernel time
from the library's events (mirt_ctx_trace_stats), median of --reps launches after a warm-up, rays and hits resident in device memory.
Beside each: the deterministic lane use nodes / (64 x wave_nodes) and the tests / nodes per ray from a counting launch.

The comparison: the render kernel's own camera rays on the same field and camera -- render_pt_hbm_kernel at 1080p x 16 spp with
num_bounces = 1, i.e. one nearest_hit_bvh per sample plus its shading -- as Mrays/s, and that launch's lane use from a counting run.
The last line per run: the 100 k tree against ten times the 10 k flat scan (the flat scan's extrapolated time).

usage: python tools/trace_rays_rates.py [--reps 5] [--fields 10000,100000,1000000] [--flat-max 10000]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import look, rtiow_field, scene_from_arrays   # noqa: E402

W, H = 1920, 1080


def pixel_centre_rays(cam) -> np.ndarray:
    """The pinhole rays through all pixel centres, image order (row 0 on top), as RAY_DTYPE records with t_max = 1000."""
    eye, hor, ver, llc = (np.asarray(a[:3], np.float32) for a in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    u = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) / np.float32(W))[None, :, None]
    v = (np.float32(1.0) - (np.arange(H, dtype=np.float32) + np.float32(0.5)) / np.float32(H))[:, None, None]
    d = (llc + u * hor + v * ver - eye).astype(np.float32).reshape(-1, 3)
    return m.make_rays(eye, d, 1000.0)


def timed(ctx, d_rays, n, d_hits, flags, reps):
    ctx.trace_rays_device(d_rays, n, d_hits, flags)
    ctx.trace_stats()                                             # warm-up, waited for
    ts = []
    for _ in range(reps):
        ctx.trace_rays_device(d_rays, n, d_hits, flags)
        ts.append(ctx.trace_stats()["kernel_ms"])
    return statistics.median(ts), ts


def field(n: int, reps: int, flat_max: int, out: dict):
    import torch
    arr, mats, tex = rtiow_field(n, seed=n)
    sd = scene_from_arrays(look(W, H, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    ctx = m.Context(0)
    ctx.set_scene(sd, hbm=True, bvh="device")
    plan = ctx.bvh_info()["plan"]
    rays = pixel_centre_rays(sd.camera)
    n_rays = len(rays)
    orders = {"image": rays, "shuffled": rays[np.random.default_rng(1).permutation(n_rays)]}
    d_hits = torch.zeros(32 * n_rays, dtype=torch.uint8, device="cuda:0")
    for order, r in orders.items():
        d_rays = torch.from_numpy(np.ascontiguousarray(r).view(np.uint8)).to("cuda:0")
        for build in (["tree"] + (["flat"] if n <= flat_max else [])):
            for query in ("nearest", "any"):
                flags = (m.MIRT_RAYS_FLAT if build == "flat" else 0) | (m.MIRT_RAYS_ANY_HIT if query == "any" else 0)
                ms, ts = timed(ctx, d_rays.data_ptr(), n_rays, d_hits.data_ptr(), flags, reps)
                kernel = ctx.last_kernel()
                ctx.trace_rays_device(d_rays.data_ptr(), n_rays, d_hits.data_ptr(), flags | m.MIRT_RAYS_COUNT)
                st = ctx.trace_stats()
                line = {"case": "trace", "n_spheres": n, "order": order, "build": build, "query": query, "rays": n_rays, "kernel_ms": round(ms, 4),
                        "all_ms": [round(x, 4) for x in ts], "mrays_per_s": round(n_rays / ms / 1e3, 1), "hit_fraction": round(st["hits"] / st["rays"], 4),
                        "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["nodes"] / st["rays"], 2),
                        "lane_use": round(st["nodes"] / (64.0 * st["wave_nodes"]), 4) if st["wave_nodes"] else None,
                        "max_depth": plan["max_depth"], "kernel": kernel}
                print(json.dumps(line), flush=True)
                out[(n, order, build, query)] = ms
    # the render kernel's camera rays: one bounce = one nearest_hit_bvh per sample, plus its shading
    spp = 16
    p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=1)
    ctx.render(p)
    ctx.stats()
    ts = []
    for _ in range(reps):
        ctx.render(p)
        ts.append(ctx.stats()["kernel_ms"])
    ms = statistics.median(ts)
    kernel = ctx.last_kernel()
    ctx.render(m.make_params(W, H, 2, mode=m.MIRT_MODE_PT, num_bounces=1, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID))
    st = ctx.stats()
    print(json.dumps({"case": "render_first_bounce", "n_spheres": n, "rays": W * H * spp, "spp": spp, "kernel_ms": round(ms, 4),
                      "all_ms": [round(x, 4) for x in ts], "mrays_per_s": round(W * H * spp / ms / 1e3, 1),
                      "tests_per_ray": round(st["sphere_tests"] / st["rays"], 2), "nodes_per_ray": round(st["grid_cells"] / st["rays"], 2),
                      "lane_use": round(st["grid_cells"] / (64.0 * st["grid_wave_cells"]), 4) if st["grid_wave_cells"] else None,
                      "kernel": kernel, "counting_kernel": ctx.last_kernel()}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fields", default="10000,100000,1000000")
    ap.add_argument("--flat-max", type=int, default=10000, help="largest field that also runs the flat scan")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("trace_rays_rates.py measures on the GPU: no device visible")
    out = {}
    for n in (int(x) for x in a.fields.split(",")):
        field(n, a.reps, a.flat_max, out)
    tree, flat = out.get((100000, "image", "tree", "nearest")), out.get((10000, "image", "flat", "nearest"))
    if tree and flat:
        print(json.dumps({"case": "tree_100k_vs_flat_extrapolated", "tree_100k_ms": round(tree, 4), "flat_10k_ms": round(flat, 4),
                          "flat_100k_extrapolated_ms": round(10 * flat, 3), "ratio": round(10 * flat / tree, 1),
                          "tree_beats_flat": bool(tree < 10 * flat)}), flush=True)


if __name__ == "__main__":
    main()
