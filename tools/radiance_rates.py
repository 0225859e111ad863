#!/usr/bin/env python3
"""Radiance-query rates (mirt_ctx_trace_radiance_device): one JSON line per case, written to
profiles/r13_radiance_rates.jsonl and printed.

Worlds: the RTIOW-style fields of tests/hbm_worlds.py at 484 and at 1 M spheres (--spheres), set with MIRT_SCENE_HBM, the tree built
on the device.  For every world and for 2 and 16 samples per pixel (8 bounces) three launches are timed on ONE context in alternating
windows:
  render     the yardstick: mirt_ctx_render_device of a 1920 x 1080 frame, the default strip kernel
  coherent   mirt_ctx_trace_radiance_device over the 1920 x 1080 CENTRE rays of the same camera in image order, stream = pixel index:
             the same tree and statistically the same paths, plus 32 bytes read and 32 bytes written per ray
  shuffled   the same rays in a random order (seeded): what the coherence of neighbouring rays is worth
A window is as many UNTIMED launches (mirt_ctx_set_timing off: the library records no event pair) as add up to about --window-ms,
queued back to back on one torch stream between two device events; its figure is the events' time over the launches.  After a
warm-up window of each, the median of --reps windows is reported, with every window's figure beside it.
  --sort     adds coherent_sort and shuffled_sort: the same two batches with MIRT_RADIANCE_SORT
  --pool     adds, for every query variant, its twin with MIRT_RADIANCE_POOL (<variant>_pool) and render_pool, the frame
             with MIRT_FLAG_KERNEL_POOL -- the pooled pair's own yardstick -- in the same alternating windows
  --pool-blocks N|resident   (with --pool) adds <variant>_pool_capped: the pooled call on a SECOND context of the same scene created under
             MIRT_RADIANCE_POOL_BLOCKS=N -- `resident`: as many blocks as mirt_bvh_pool_plan keeps on the device at once -- so that its
             waves stride over the units, against one unit per wave, in the same alternating windows
Every variant's records are compared with the coherent batch's, byte for byte, in the caller's order ("same_records").

usage: python tools/radiance_rates.py [--reps 5] [--spheres 484,1000000] [--spp 2,16] [--window-ms 200] [--sort] [--pool [--pool-blocks N|resident]]
                                      [--out profiles/r13_radiance_rates.jsonl]"""
from __future__ import annotations

import argparse
import json
import os
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


def centre_rays(cam) -> np.ndarray:
    """The centre rays of all pixels in image order as RADIANCE_RAY_DTYPE records, stream = pixel index (for timing: numpy's
    arithmetic, not the renderer's to the bit)."""
    eye, hor, ver, llc = (np.asarray(a[:3], np.float32) for a in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    u = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(W)))[None, :, None]
    v = (np.float32(1.0) - (np.arange(H, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(H)))[:, None, None]
    d = (llc + u * hor + v * ver - eye).astype(np.float32).reshape(-1, 3)
    return m.make_radiance_rays(eye, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spheres", default="484,1000000")
    ap.add_argument("--spp", default="2,16")
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--sort", action="store_true", help="also time both batches with MIRT_RADIANCE_SORT")
    ap.add_argument("--pool", action="store_true", help="also time every query with MIRT_RADIANCE_POOL, and the frame with MIRT_FLAG_KERNEL_POOL")
    ap.add_argument("--pool-blocks", default="", help="--pool: also time the pooled call with its grid capped at N blocks, or `resident`")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_radiance_rates.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("radiance_rates.py measures on the GPU: no device visible")
    npix = W * H
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    stream = torch.cuda.Stream(device="cuda:0")
    d_img = torch.zeros(4 * npix, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0")
    for n in [int(x) for x in a.spheres.split(",") if x]:
        arr, mats, tex = rtiow_field(n, seed=n)
        eye = (13, 2, 3) if n < 5000 else (40, 6, 30)
        sd = scene_from_arrays(look(W, H, eye, (0, 0, 0), vfov=25 if n < 5000 else 35), arr, mats, tex)
        ctx = m.Context(0)
        ctx.set_scene(sd, hbm=True, bvh="device")
        depth = ctx.bvh_info()["plan"]["max_depth"]
        capped, cap = None, 0
        if a.pool and a.pool_blocks:                                # the knob is read when a context is created
            plan = m.bvh_pool_plan(depth)
            cap = (plan["waves_per_cu"] // (plan["threads"] // 64) * torch.cuda.get_device_properties(0).multi_processor_count
                   if a.pool_blocks == "resident" else int(a.pool_blocks))
            os.environ["MIRT_RADIANCE_POOL_BLOCKS"] = str(cap)
            capped = m.Context(0)
            del os.environ["MIRT_RADIANCE_POOL_BLOCKS"]
            capped.set_scene(sd, hbm=True, bvh="device")
        rays = centre_rays(sd.camera)
        order = np.random.default_rng(1).permutation(npix)
        d_rays = {"coherent": torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0"),
                  "shuffled": torch.from_numpy(np.ascontiguousarray(rays[order]).view(np.uint8).copy()).to("cuda:0")}
        for spp in [int(x) for x in a.spp.split(",") if x]:
            p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
            launch = {"render": lambda: ctx.render_device(p, d_img.data_ptr(), d_img.numel(), stream=stream.cuda_stream)}
            if a.pool:
                pp = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8, flags=m.MIRT_FLAG_KERNEL_POOL)
                launch["render_pool"] = lambda: ctx.render_device(pp, d_img.data_ptr(), d_img.numel(), stream=stream.cuda_stream)
            for sort in ((False, True) if a.sort else (False,)):
                for pool in ((False, True) if a.pool else (False,)):
                    for k in ("coherent", "shuffled"):
                        launch[k + ("_sort" if sort else "") + ("_pool" if pool else "")] = (
                            lambda k=k, sort=sort, pool=pool: ctx.trace_radiance_device(d_rays[k].data_ptr(), npix, d_out.data_ptr(), spp, num_bounces=8,
                                                                                        stream=stream.cuda_stream, sort=sort, pool=pool))
                        if pool and capped is not None:
                            launch[k + ("_sort" if sort else "") + "_pool_capped"] = (
                                lambda k=k, sort=sort: capped.trace_radiance_device(d_rays[k].data_ptr(), npix, d_out.data_ptr(), spp, num_bounces=8,
                                                                                    stream=stream.cuda_stream, sort=sort, pool=True))

            def window(fn, count):
                """`count` launches back to back between two device events -> ms per launch."""
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(count):
                    fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / count

            kernels, counts, sums, same, reference = {}, {}, {}, {}, None
            ctx.set_timing(False)
            if capped is not None:
                capped.set_timing(False)
            for k, fn in launch.items():                            # warm-up: code objects, then one window that also sizes the windows
                window(fn, 1)
                kernels[k] = (capped if k.endswith("_capped") else ctx).last_kernel()
                counts[k] = max(1, int(round(a.window_ms / max(window(fn, 2), 1e-3))))
                window(fn, counts[k])
                if not k.startswith("render"):
                    rec = d_out.cpu().numpy().view(m.RADIANCE_DTYPE)
                    if k.startswith("shuffled"):
                        rec = rec[np.argsort(order)]                 # back to image order
                    sums[k] = rec["sum"].sum(0).tolist()
                    if reference is None:
                        reference = rec.tobytes()                   # "coherent" comes first
                    same[k] = rec.tobytes() == reference
            t = {k: [] for k in launch}
            for _ in range(a.reps):                                 # alternating windows
                for k, fn in launch.items():
                    t[k].append(window(fn, counts[k]))
            ctx.set_timing(True)
            if capped is not None:
                capped.set_timing(True)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({"case": "radiance", "world": f"rtiow_field({n})", "n_spheres": n, "max_depth": depth, "width": W, "height": H, "rays": npix, "spp": spp,
                  "num_bounces": 8, "render_us": round(med["render"] * 1e3, 1), "coherent_us": round(med["coherent"] * 1e3, 1),
                  "shuffled_us": round(med["shuffled"] * 1e3, 1), "coherent_over_render": round(med["coherent"] / med["render"], 3),
                  "shuffled_over_coherent": round(med["shuffled"] / med["coherent"], 3),
                  "msamples_per_s": {k: round(npix * spp / v / 1e3, 1) for k, v in med.items()},
                  "same_sums_in_either_order": sums["coherent"] == sums["shuffled"], "same_records": same,
                  "us": {k: round(v * 1e3, 1) for k, v in med.items()},
                  "pool_over_plain": {k: round(med[k + "_pool"] / med[k], 3) for k in med if k + "_pool" in med},
                  "capped_over_one_unit_per_wave": {k: round(med[k + "_capped"] / med[k], 3) for k in med if k + "_capped" in med}, "pool_blocks_cap": cap,
                  "kernels": kernels, "launches_per_window": counts,
                  "window_ms": a.window_ms, "reps": a.reps, "all_us": {k: [round(x * 1e3, 1) for x in v] for k, v in t.items()}})
        ctx.close()
        if capped is not None:
            capped.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
