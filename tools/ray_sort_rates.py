#!/usr/bin/env python3
"""What MIRT_RADIANCE_SORT / MIRT_RAYS_SORT cost and gain: one JSON line per workload, written to
profiles/r14_ray_sort_rates.jsonl and printed.  The method is tools/radiance_rates.py's.

Worlds: the RTIOW-style fields of tests/hbm_worlds.py at 484 and at 1 M spheres (--spheres), set with MIRT_SCENE_HBM, the tree built
on the device; rays: the 1920 x 1080 centre rays of DESIGN.md 10.9's cameras.  Workloads per world: mirt_ctx_trace_radiance_device at
2 and 16 samples per ray (8 bounces), and the same rays through mirt_ctx_trace_rays_device for the nearest hit and for any hit
(t_max 1000).  Four variants of every workload are timed on ONE context in alternating windows:
  in_order           the rays in image order, without the flag
  in_order_sorted    the same batch with the flag: what sorting costs a caller whose rays are coherent already
  shuffled           the rays in a random order (seeded), without the flag: the parent's code object, the baseline of the comparison
  shuffled_sorted    the same shuffled batch with the flag
The sorted times include the code kernel and the radix sort: a window is as many UNTIMED calls (mirt_ctx_set_timing off) as add up to
about --window-ms, queued back to back on one torch stream between two device events; its figure is the events' time over the calls.
After a warm-up window of each, the median of --reps windows is reported with every window's figure beside it.  "gain" is stated only
where the sorted median beats the unsorted median of the same batch by more than the spread (max - min) of the windows of either.

usage: python tools/ray_sort_rates.py [--reps 5] [--spheres 484,1000000] [--spp 2,16] [--window-ms 200] [--out profiles/r14_ray_sort_rates.jsonl]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import look, rtiow_field, scene_from_arrays   # noqa: E402
from radiance_rates import H, W, centre_rays                # noqa: E402

VARIANTS = ("in_order", "in_order_sorted", "shuffled", "shuffled_sorted")


def verdict(sorted_us, plain_us):
    """("gain" | "loss" | "within the spread", sorted median / unsorted median)."""
    ms, mp = statistics.median(sorted_us), statistics.median(plain_us)
    spread = max(max(sorted_us) - min(sorted_us), max(plain_us) - min(plain_us))
    return ("gain" if mp - ms > spread else "loss" if ms - mp > spread else "within the spread"), round(ms / mp, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spheres", default="484,1000000")
    ap.add_argument("--spp", default="2,16")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14_ray_sort_rates.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ray_sort_rates.py measures on the GPU: no device visible")
    npix = W * H
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    stream = torch.cuda.Stream(device="cuda:0")
    d_out = torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0")

    def window(fn, count):
        """`count` calls back to back between two device events -> ms per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(count):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / count

    for n in [int(x) for x in a.spheres.split(",") if x]:
        arr, mats, tex = rtiow_field(n, seed=n)
        eye = (13, 2, 3) if n < 5000 else (40, 6, 30)
        sd = scene_from_arrays(look(W, H, eye, (0, 0, 0), vfov=25 if n < 5000 else 35), arr, mats, tex)
        ctx = m.Context(0)
        ctx.set_scene(sd, hbm=True, bvh="device")
        depth = ctx.bvh_info()["plan"]["max_depth"]
        rays = centre_rays(sd.camera)
        order = np.random.default_rng(1).permutation(npix)
        # MirtRadianceRay and MirtRay share origin and direction; word 3 is the stream there and t_max here
        as_rays = rays.copy().view(m.RAY_DTYPE)
        as_rays["t_max"] = 1000.0
        dev = lambda recs: torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).copy()).to("cuda:0")
        d_rad = {"in_order": dev(rays), "shuffled": dev(rays[order])}
        d_ray = {"in_order": dev(as_rays), "shuffled": dev(as_rays[order])}
        workloads = [("radiance", spp) for spp in [int(x) for x in a.spp.split(",") if x]] + [("trace_rays nearest", 0), ("trace_rays any hit", m.MIRT_RAYS_ANY_HIT)]
        for kind, arg in workloads:
            launch = {}
            for v in VARIANTS:
                batch, sort = v.split("_sorted")[0], v.endswith("_sorted")
                if kind == "radiance":
                    launch[v] = (lambda b=batch, s=sort: ctx.trace_radiance_device(d_rad[b].data_ptr(), npix, d_out.data_ptr(), arg, num_bounces=8,
                                                                                   stream=stream.cuda_stream, sort=s))
                else:
                    launch[v] = (lambda b=batch, s=sort: ctx.trace_rays_device(d_ray[b].data_ptr(), npix, d_out.data_ptr(), arg, stream=stream.cuda_stream, sort=s))
            kernels, counts, digest = {}, {}, {}
            ctx.set_timing(False)
            for v, fn in launch.items():                            # warm-up: code objects and scratch, then one window that also sizes the windows
                window(fn, 1)
                kernels[v] = ctx.last_kernel()
                counts[v] = max(1, int(round(a.window_ms / max(window(fn, 2), 1e-3))))
                window(fn, counts[v])
                rec = d_out.cpu().numpy().view(np.uint64).reshape(npix, 4)
                digest[v] = (rec if v.startswith("in_order") else rec[np.argsort(order)]).sum(0, dtype=np.uint64).tolist()
            t = {v: [] for v in launch}
            for _ in range(a.reps):                                 # alternating windows
                for v, fn in launch.items():
                    t[v].append(window(fn, counts[v]))
            ctx.set_timing(True)
            us = {v: [round(x * 1e3, 1) for x in xs] for v, xs in t.items()}
            med = {v: statistics.median(xs) for v, xs in us.items()}
            shuffled_verdict, shuffled_ratio = verdict(us["shuffled_sorted"], us["shuffled"])
            in_order_verdict, in_order_ratio = verdict(us["in_order_sorted"], us["in_order"])
            emit({"case": "ray_sort", "workload": kind, "spp": arg if kind == "radiance" else None, "world": f"rtiow_field({n})", "n_spheres": n,
                  "max_depth": depth, "width": W, "height": H, "rays": npix, "num_bounces": 8 if kind == "radiance" else None,
                  "median_us": med, "shuffled_over_in_order": round(med["shuffled"] / med["in_order"], 3),
                  "shuffled_sorted_over_shuffled": shuffled_ratio, "shuffled_verdict": shuffled_verdict,
                  "in_order_sorted_over_in_order": in_order_ratio, "in_order_verdict": in_order_verdict,
                  "same_records_in_all_four": all(digest[v] == digest["in_order"] for v in VARIANTS), "kernels": kernels,
                  "calls_per_window": counts, "window_ms": a.window_ms, "reps": a.reps, "all_us": us})
        ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
