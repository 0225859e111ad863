#!/usr/bin/env python3
"""Feature-frame rates (mirt_ctx_render_features_device): one JSON line per case, written to
profiles/r12_feature_rates.jsonl and printed.

The frame is 1920 x 1080 over the RTIOW-style field of 100 k spheres of tools/hbm_scene_rates.py (camera of DESIGN.md 10.2), the tree
built on the device.  Every figure is the median of --reps runs after a warm-up:
  feature      us per feature frame at spp 0, 1, 2 and 4 (kernel time from the library's events, mirt_ctx_trace_stats), the records
               resident in device memory; at spp 0 also the flat-scan build when --flat is given (100 k tests per ray: slow)
  trace_route  the route a feature frame replaces: mirt_ctx_trace_rays_device over the same centre rays -- its kernel time, and
               beside it, separately, the upload of the 32-byte rays and the download of the 32-byte hits (wall clock around a
               synchronised copy), which a feature frame does not pay
  render       mirt_ctx_render_device at spp 1, 2 and 4 with the default 8 bounces, for scale

usage: python tools/feature_frame_rates.py [--reps 5] [--spheres 100000] [--flat] [--out profiles/r12_feature_rates.jsonl]"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import look, rtiow_field, scene_from_arrays   # noqa: E402

W, H = 1920, 1080


def centre_rays(cam) -> np.ndarray:
    """The centre rays of all pixels in image order as RAY_DTYPE records (for timing: numpy's arithmetic, not the kernel's to the bit)."""
    eye, hor, ver, llc = (np.asarray(a[:3], np.float32) for a in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    u = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(W)))[None, :, None]
    v = (np.float32(1.0) - (np.arange(H, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(H)))[:, None, None]
    d = (llc + u * hor + v * ver - eye).astype(np.float32).reshape(-1, 3)
    return m.make_rays(eye, d, 1000.0)


def median_of(fn, reps):
    fn()                                                          # warm-up
    ts = [fn() for _ in range(reps)]
    return statistics.median(ts), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spheres", type=int, default=100000)
    ap.add_argument("--flat", action="store_true", help="also time the flat-scan build at spp 0")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_feature_rates.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("feature_frame_rates.py measures on the GPU: no device visible")
    n = a.spheres
    arr, mats, tex = rtiow_field(n, seed=n)
    sd = scene_from_arrays(look(W, H, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    ctx = m.Context(0)
    ctx.set_scene(sd, hbm=True, bvh="device")
    depth = ctx.bvh_info()["plan"]["max_depth"]
    npix = W * H
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    d_out = torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0")
    hit_fraction = None
    for spp, flat in [(0, False), (1, False), (2, False), (4, False)] + ([(0, True)] if a.flat else []):
        p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT)

        def run():
            ctx.render_features_device(p, d_out.data_ptr(), d_out.numel(), flat=flat)
            return ctx.trace_stats()["kernel_ms"]
        ms, ts = median_of(run, a.reps)
        if hit_fraction is None:
            rec = d_out.cpu().numpy().view(m.FEATURE_DTYPE)
            hit_fraction = float((rec["sphere"] != m.MIRT_RAY_MISS).mean())
        emit({"case": "feature", "n_spheres": n, "width": W, "height": H, "spp": spp, "build": "flat" if flat else "tree", "rays_per_pixel": 1 if spp == 0 else spp + 1,
              "frame_us": round(ms * 1e3, 1), "all_ms": ts, "mrays_per_s": round(npix * (1 if spp == 0 else spp + 1) / ms / 1e3, 1),
              "hit_fraction": round(hit_fraction, 4), "max_depth": depth, "kernel": ctx.last_kernel()})

    # the route this replaces: rays made on the host, uploaded, traced, the hits downloaded
    rays = centre_rays(sd.camera)
    h_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8)).pin_memory()
    d_rays = torch.empty_like(h_rays, device="cuda:0")
    d_hits = torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0")
    h_hits = torch.empty(32 * npix, dtype=torch.uint8).pin_memory()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def trace():
        ctx.trace_rays_device(d_rays.data_ptr(), npix, d_hits.data_ptr(), 0)
        return ctx.trace_stats()["kernel_ms"]
    up, up_all = median_of(lambda: wall(lambda: d_rays.copy_(h_rays, non_blocking=True)), a.reps)
    kern, kern_all = median_of(trace, a.reps)
    down, down_all = median_of(lambda: wall(lambda: h_hits.copy_(d_hits, non_blocking=True)), a.reps)
    emit({"case": "trace_route", "n_spheres": n, "rays": npix, "kernel_us": round(kern * 1e3, 1), "upload_us": round(up * 1e3, 1), "download_us": round(down * 1e3, 1),
          "bytes_each_way": 32 * npix, "pinned_host_memory": True, "kernel_all_ms": kern_all, "upload_all_ms": up_all, "download_all_ms": down_all,
          "kernel": ctx.last_kernel()})

    d_img = torch.zeros(4 * npix, dtype=torch.uint8, device="cuda:0")
    for spp in (1, 2, 4):
        p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT)

        def run():
            ctx.render_device(p, d_img.data_ptr(), d_img.numel())
            return ctx.stats()["kernel_ms"]
        ms, ts = median_of(run, a.reps)
        emit({"case": "render", "n_spheres": n, "spp": spp, "num_bounces": int(p.num_bounces), "frame_us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
