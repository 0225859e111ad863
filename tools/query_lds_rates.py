#!/usr/bin/env python3
"""Rates of the MIRT_QUERY_LDS queries against the same queries on the same world held as a MIRT_SCENE_HBM scene
with a device-built tree -- rtiow_field(484) at 1920 x 1080, held by two contexts in ONE process.  The method is 10.15's
(tools/adaptive_rates.py --lds): per case the variants run in alternating windows, a warm-up of every variant first, then --reps rounds;
the figure is the median window, every window's figure stands beside it.  A window is --count device-path calls back to back between two
events on one torch stream.

  features     a feature frame at spp 0 and 2:            lds (grid), lds_flat, hbm (tree)
  rays         2 M centre rays, nearest hit and any-hit:  lds (grid), lds_flat, hbm (tree), hbm_sorted is not run (the rays are coherent)
  radiance     the same rays at 2 and 16 spp, 8 bounces:  lds (grid), hbm (tree), hbm_pool (MIRT_RADIANCE_POOL)
  render       what the flag exists for: the time of render() -- a uniform --render-spp frame -- after pick(lds=True), where the scene is
               still in LDS, against render() after today's pick(), which has set it again as an HBM scene.  Two Raytracers, alternating.

Before anything is timed every LDS variant's bytes are compared with the HBM variant's.  Appends JSON lines to
profiles/r24_query_lds_rates.jsonl (or --out)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
W, H, BOUNCES = 1920, 1080, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=4, help="calls per window")
    ap.add_argument("--cases", default="features,rays,radiance,render")
    ap.add_argument("--render-spp", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r24_query_lds_rates.jsonl"))
    ap.add_argument("--note", default="", help="copied into every line")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("query_lds_rates.py measures on the GPU: no device visible")
    import weekend_raytracer_wgpu_amd as m
    from hbm_worlds import look, rtiow_field, scene_from_arrays

    def emit(line):
        if a.note:
            line["note"] = a.note
        print(json.dumps(line), flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    cases = [c for c in a.cases.split(",") if c]
    stream = torch.cuda.Stream(device="cuda:0")
    npix = W * H
    arr, mats, tex = rtiow_field(484, seed=484)
    cam = look(W, H, (13, 2, 3), (0, 0, 0), vfov=25)
    sd = scene_from_arrays(cam, arr, mats, tex)
    lds, hbm = m.Context(0), m.Context(0)
    lds.set_scene(sd)
    hbm.set_scene(sd, hbm=True, bvh="device")
    base = {"world": "rtiow_field(484)", "width": W, "height": H, "reps": a.reps, "calls_per_window": a.count}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.count):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.count

    def compare(case, variants, outputs, reference):
        """variants: name -> (fn, context); outputs: name -> device tensor.  Same bytes first, then alternating windows."""
        for name, (fn, _) in variants.items():
            fn()
        stream.synchronize()
        want = outputs[reference].cpu().numpy()
        same = {name: bool(np.array_equal(t.cpu().numpy(), want)) for name, t in outputs.items()}
        for name, (fn, _) in variants.items():          # warm-up
            window(fn)
        t = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, (fn, _) in variants.items():
                t[name].append(window(fn))
        emit({**base, **case, "ms": {k: round(statistics.median(v), 4) for k, v in t.items()}, "windows_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
              "same_bytes_as_" + reference: same, "kernels": {name: (fn(), stream.synchronize(), c.last_kernel())[2] for name, (fn, c) in variants.items()}})

    s = stream.cuda_stream
    if "features" in cases:
        outs = {k: torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0") for k in ("lds", "lds_flat", "hbm")}
        for spp in (0, 2):
            p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT)
            compare({"case": "features", "spp": spp},
                    {"lds": (lambda: lds.render_features_device(p, outs["lds"].data_ptr(), 32 * npix, stream=s, lds=True), lds),
                     "lds_flat": (lambda: lds.render_features_device(p, outs["lds_flat"].data_ptr(), 32 * npix, flat=True, stream=s, lds=True), lds),
                     "hbm": (lambda: hbm.render_features_device(p, outs["hbm"].data_ptr(), 32 * npix, stream=s), hbm)}, outs, "hbm")
    if "rays" in cases or "radiance" in cases:
        ys, xs = np.divmod(np.arange(npix), W)
        import feature_ref as fr
        o, d = fr.centre_rays(cam, W, H, xs, ys)
    if "rays" in cases:
        d_rays = torch.from_numpy(np.ascontiguousarray(m.make_rays(o, d, 1000.0)).view(np.uint8)).to("cuda:0")
        outs = {k: torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0") for k in ("lds", "lds_flat", "hbm")}
        for what, flags in (("nearest", 0), ("any_hit", m.MIRT_RAYS_ANY_HIT)):
            compare({"case": "rays", "n_rays": npix, "query": what},
                    {"lds": (lambda: lds.trace_rays_device(d_rays.data_ptr(), npix, outs["lds"].data_ptr(), flags, stream=s, lds=True), lds),
                     "lds_flat": (lambda: lds.trace_rays_device(d_rays.data_ptr(), npix, outs["lds_flat"].data_ptr(), flags | m.MIRT_RAYS_FLAT, stream=s, lds=True), lds),
                     "hbm": (lambda: hbm.trace_rays_device(d_rays.data_ptr(), npix, outs["hbm"].data_ptr(), flags, stream=s), hbm)}, outs, "hbm")
    if "radiance" in cases:
        d_rays = torch.from_numpy(np.ascontiguousarray(m.make_radiance_rays(o, d, np.arange(npix))).view(np.uint8)).to("cuda:0")
        outs = {k: torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0") for k in ("lds", "hbm", "hbm_pool")}
        for spp in (2, 16):
            kw = dict(num_bounces=BOUNCES, stream=s)
            compare({"case": "radiance", "n_rays": npix, "spp": spp, "num_bounces": BOUNCES},
                    {"lds": (lambda: lds.trace_radiance_device(d_rays.data_ptr(), npix, outs["lds"].data_ptr(), spp, lds=True, **kw), lds),
                     "hbm": (lambda: hbm.trace_radiance_device(d_rays.data_ptr(), npix, outs["hbm"].data_ptr(), spp, **kw), hbm),
                     "hbm_pool": (lambda: hbm.trace_radiance_device(d_rays.data_ptr(), npix, outs["hbm_pool"].data_ptr(), spp, pool=True, **kw), hbm)}, outs, "hbm")
    if "render" in cases:
        import time
        scene, camera = m.scenes.rtiow_final() if hasattr(m.scenes, "rtiow_final") else m.scenes.three_spheres()
        rp = m.RenderParams(camera=camera, viewport_size=(W, H),
                            sampling=m.SamplingParams(max_samples_per_pixel=a.render_spp, num_samples_per_pixel=a.render_spp, num_bounces=BOUNCES))
        stay, move = m.Raytracer(scene, rp, device=0), m.Raytracer(scene, rp, device=0)
        a_hit, b_hit = stay.pick(W // 2, H // 2, lds=True), move.pick(W // 2, H // 2)

        def frame(rt):
            rt._ctx.synchronize()
            t0 = time.perf_counter()
            img = rt.render()
            return (time.perf_counter() - t0) * 1e3, img

        imgs = {k: frame(rt)[1] for k, rt in (("after_pick_lds", stay), ("after_pick", move))}       # warm-up
        t = {"after_pick_lds": [], "after_pick": []}
        for _ in range(a.reps):
            for k, rt in (("after_pick_lds", stay), ("after_pick", move)):
                t[k].append(frame(rt)[0])
        emit({**base, "case": "render", "scene": "rtiow_final, %d spheres" % len(scene.spheres), "spp": a.render_spp, "num_bounces": BOUNCES,
              "ms": {k: round(statistics.median(v), 3) for k, v in t.items()}, "windows_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
              "kernel_ms": {"after_pick_lds": round(stay._ctx.stats()["kernel_ms"], 3), "after_pick": round(move._ctx.stats()["kernel_ms"], 3)},
              "kernels": {"after_pick_lds": stay._ctx.last_kernel(), "after_pick": move._ctx.last_kernel()},
              "same_pick": bool((a_hit is None) == (b_hit is None) and (a_hit is None or (a_hit["sphere"] == b_hit["sphere"] and a_hit["t"] == b_hit["t"]))),
              "same_image": bool(np.array_equal(imgs["after_pick_lds"], imgs["after_pick"])), "scene_in_lds": [not stay._hbm, not move._hbm]})
        stay.close()
        move.close()
    lds.close()
    hbm.close()


if __name__ == "__main__":
    main()
