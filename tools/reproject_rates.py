#!/usr/bin/env python3
"""Reprojection rates (mirt_ctx_reproject_device): one JSON line per case, written to
profiles/r27_reproject_rates.jsonl and printed.

The frames are 1920 x 1080 over rtiow_field(3000) as a MIRT_SCENE_HBM scene: the previous frame from the camera of the feature
fixture, the current one from a camera moved a little (the pair of tests/test_gpu_reproject.py).  Each is one progressive frame of
2 spp, its feature frame at spp 2 and the a-trous filter at 3 levels to float32, all resident in device memory.  Every kernel figure
is the median of --reps calls after a warm-up, between the library's device events (mirt_ctx_trace_stats().kernel_ms; MirtStats for
the frame).
  reproject    us per call with and without the clamp, with and without the RGBA8 plane; `history` is the share of pixels that found
               history.  floor_us: the bytes of a call over the measured float4-copy rate (6.29 TB/s) -- 16 + 32 bytes of the current
               frame, 4 x 48 bytes of taps as an upper bound, 16 (+ 4) bytes out; the clamp's eight neighbours are not counted (they
               are the lanes' own records, from L2)
  scale        mirt_ctx_accum_frame_device (2 spp), mirt_ctx_render_features_device (spp 2) and mirt_ctx_denoise_device (3 levels,
               float32) on the same scene: what a temporal frame runs before the reprojection
  chain        the four calls of a temporal frame queued on one stream and waited for once, wall clock, with and without the
               reprojection (without: the denoiser writes RGBA8 itself)

usage: python tools/reproject_rates.py [--reps 5] [--out profiles/r27_reproject_rates.jsonl]"""
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

import numpy as np                                          # noqa: E402
import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import look, rtiow_field, scene_from_arrays   # noqa: E402

W, H = 1920, 1080
COPY_TBS = 6.29                                             # float4 copy, measured


def median_of(fn, reps):
    fn()                                                    # warm-up
    ts = [fn() for _ in range(reps)]
    return statistics.median(ts), [round(t, 4) for t in ts]


def floor_us(rgba8):
    return W * H * (16 + 32 + 4 * 48 + 16 + (4 if rgba8 else 0)) / (COPY_TBS * 1e12) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r27_reproject_rates.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reproject_rates.py measures on the GPU: no device visible")
    npix = W * H
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    plane = lambda size: torch.zeros(size * npix, dtype=torch.uint8, device="cuda:0")
    d_guides, d_colour = [plane(32), plane(32)], [plane(16), plane(16)]
    d_out, d_img = plane(16), plane(4)
    cams = [look(W, H, (13, 2, 3), (0, 0.5, 0), vfov=25), look(W, H, (12.8, 2.1, 3.3), (0, 0.5, 0), vfov=25)]
    arr, mats, tex = rtiow_field(3000)
    ctx = m.Context(0)
    ctx.set_scene(scene_from_arrays(cams[0], arr, mats, tex), hbm=True, bvh="device")
    to_f32 = m.make_denoise_params("accum", levels=3, f32=True)
    to_rgba8 = m.make_denoise_params("accum", levels=3)
    tone = m.make_params(W, H, 0, mode=m.MIRT_MODE_PT)

    def frame_of(k):
        p = m.make_params(W, H, 2, mode=m.MIRT_MODE_PT, seed=k)
        ctx.set_camera(cams[k])
        ctx.accum_reset(p)
        ctx.accum_frame_device(p, d_img.data_ptr())
        ctx.render_features_device(p, d_guides[k].data_ptr(), 32 * npix)
        ctx.denoise_device(tone, to_f32, d_guides[k].data_ptr(), 32 * npix, d_colour[k].data_ptr(), 16 * npix)
        ctx.synchronize()
        return p

    frame_of(0)
    p = frame_of(1)

    # the scale: what a temporal frame runs before the reprojection (camera 1, whose sums are in place)
    def frame():
        ctx.accum_frame_device(p, d_img.data_ptr())
        return ctx.stats()["kernel_ms"]
    ms, ts = median_of(frame, a.reps)
    emit({"case": "scale", "what": "accum_frame_device", "spp": 2, "us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})

    def feat():
        ctx.render_features_device(p, d_guides[1].data_ptr(), 32 * npix)
        return ctx.trace_stats()["kernel_ms"]
    ms, ts = median_of(feat, a.reps)
    emit({"case": "scale", "what": "render_features_device", "spp": 2, "us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})

    def den():
        ctx.denoise_device(tone, to_f32, d_guides[1].data_ptr(), 32 * npix, d_out.data_ptr(), 16 * npix)
        return ctx.trace_stats()["kernel_ms"]
    ms, ts = median_of(den, a.reps)
    emit({"case": "scale", "what": "denoise_device", "levels": 3, "out": "f32", "us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})

    # the call itself
    for clamp in (True, False):
        r = m.make_reproject_params(cams[0], cams[1], clamp=clamp)
        for rgba8 in (True, False):
            def run():
                ctx.reproject_device(tone, r, d_colour[1].data_ptr(), d_guides[1].data_ptr(), d_colour[0].data_ptr(), d_guides[0].data_ptr(), d_out.data_ptr(), npix,
                                     d_out_rgba8=d_img.data_ptr() if rgba8 else None)
                return ctx.trace_stats()["kernel_ms"]
            ms, ts = median_of(run, a.reps)
            ctx.synchronize()
            have = float((d_out.cpu().numpy().view(np.float32).reshape(-1, 4)[:, 3] != 1).mean())
            fl = floor_us(rgba8)
            emit({"case": "reproject", "clamp": clamp, "rgba8": rgba8, "us": round(ms * 1e3, 1), "all_ms": ts, "floor_us": round(fl, 1),
                  "times_floor": round(ms * 1e3 / fl, 2), "history": round(have, 4), "kernel": ctx.last_kernel()})

    # a camera that does not move: every tap of a wave is coalesced
    r = m.make_reproject_params(cams[1], cams[1])

    def still():
        ctx.reproject_device(tone, r, d_colour[1].data_ptr(), d_guides[1].data_ptr(), d_colour[1].data_ptr(), d_guides[1].data_ptr(), d_out.data_ptr(), npix,
                             d_out_rgba8=d_img.data_ptr())
        return ctx.trace_stats()["kernel_ms"]
    ms, ts = median_of(still, a.reps)
    emit({"case": "reproject", "clamp": True, "rgba8": True, "camera": "equal", "us": round(ms * 1e3, 1), "all_ms": ts, "floor_us": round(floor_us(True), 1),
          "times_floor": round(ms * 1e3 / floor_us(True), 2), "kernel": ctx.last_kernel()})

    # the chain of a temporal frame on one stream, wall clock
    stream = torch.cuda.Stream(device="cuda:0")
    st = stream.cuda_stream
    r = m.make_reproject_params(cams[0], cams[1])
    for reproject in (True, False):
        def chain():
            torch.cuda.synchronize()
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.accum_reset(p)
            ctx.accum_frame_device(p, d_img.data_ptr(), st)
            ctx.render_features_device(p, d_guides[1].data_ptr(), 32 * npix, stream=st)
            if reproject:
                ctx.denoise_device(tone, to_f32, d_guides[1].data_ptr(), 32 * npix, d_colour[1].data_ptr(), 16 * npix, st)
                ctx.reproject_device(tone, r, d_colour[1].data_ptr(), d_guides[1].data_ptr(), d_colour[0].data_ptr(), d_guides[0].data_ptr(), d_out.data_ptr(), npix,
                                     d_out_rgba8=d_img.data_ptr(), stream=st)
            else:
                ctx.denoise_device(tone, to_rgba8, d_guides[1].data_ptr(), 32 * npix, d_img.data_ptr(), 4 * npix, st)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3
        ms, ts = median_of(chain, a.reps)
        emit({"case": "chain", "reproject": reproject, "wall_us": round(ms * 1e3, 1), "all_ms": ts,
              "what": "accum_reset + accum_frame_device + render_features_device + denoise_device" + (" + reproject_device" if reproject else " (RGBA8)")})
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
