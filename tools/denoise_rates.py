#!/usr/bin/env python3
"""Denoise rates (mirt_ctx_denoise_device): one JSON line per case, written to profiles/r26_denoise_rates.jsonl and
printed.

The frame is 1920 x 1080 over rtiow_field(3000) as a MIRT_SCENE_HBM scene (the camera of the feature fixture); the sums are two
progressive frames of 2 spp (source accum) or one adaptive step of 2 spp (source adapt), the guides a feature frame at spp 2, all
resident in device memory.  Every figure is the median of --reps calls after a warm-up, between the library's device events
(mirt_ctx_trace_stats().kernel_ms: the first through the last kernel of a call).
  denoise      us per call at levels 3 and 5, both sources, RGBA8 and float32 output, in the shipped choice of shapes
  level        us per call at levels 1 .. 6 with every level direct, and with ONLY the last level staged (MIRT_DENOISE_STAGED, read when
               a context is created): the two differ in the shape of that one level, epilogue included.  `added_us` is the call minus
               the all-direct call of one level fewer: what the level adds (its kernel, and the epilogue moving one level up)
  scale        a 2-spp mirt_ctx_accum_frame_device and mirt_ctx_render_features_device at spp 0 and 2 on the same scene
  floor        the bytes of a call over the measured copy rate (6.29 TB/s): 48 bytes per pixel per level, the prepare kernel's reads and
               writes, the epilogue's guide read and output

usage: python tools/denoise_rates.py [--reps 5] [--out profiles/r26_denoise_rates.jsonl]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import weekend_raytracer_wgpu_amd as m                      # noqa: E402
from hbm_worlds import look, rtiow_field, scene_from_arrays   # noqa: E402

W, H = 1920, 1080
COPY_TBS = 6.29                                             # float4 copy, measured


def median_of(fn, reps):
    fn()                                                    # warm-up
    ts = [fn() for _ in range(reps)]
    return statistics.median(ts), [round(t, 4) for t in ts]


def floor_us(levels, source, f32):
    npix = W * H
    prepare = (24 if source == "accum" else 64) + 32 + 32
    return npix * (prepare + 48 * levels - 16 + 16 + (16 if f32 else 4)) / (COPY_TBS * 1e12) * 1e6


def context(staged=None):
    """A context with the frame's sums and records in place; staged: the MIRT_DENOISE_STAGED mask, None for the shipped choice."""
    if staged is None:
        os.environ.pop("MIRT_DENOISE_STAGED", None)
    else:
        os.environ["MIRT_DENOISE_STAGED"] = str(staged)
    arr, mats, tex = rtiow_field(3000)
    ctx = m.Context(0)
    ctx.set_scene(scene_from_arrays(look(W, H, (13, 2, 3), (0, 0.5, 0), vfov=25), arr, mats, tex), hbm=True, bvh="device")
    p = m.make_params(W, H, 2, mode=m.MIRT_MODE_PT)
    ctx.accum_reset(p)
    ctx.adapt_reset(p)
    ctx.adapt_step(p, m.make_adapt_params(2, 2, 0))
    ctx.synchronize()
    return ctx, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-level", type=int, default=6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r26_denoise_rates.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("denoise_rates.py measures on the GPU: no device visible")
    npix = W * H
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    d_guides = torch.zeros(32 * npix, dtype=torch.uint8, device="cuda:0")
    d_out = torch.zeros(16 * npix, dtype=torch.uint8, device="cuda:0")
    d_img = torch.zeros(4 * npix, dtype=torch.uint8, device="cuda:0")

    def denoise_ms(ctx, p, source, levels, f32):
        d = m.make_denoise_params(source, levels=levels, f32=f32)

        def run():
            ctx.denoise_device(p, d, d_guides.data_ptr(), d_guides.numel(), d_out.data_ptr(), d_out.numel())
            return ctx.trace_stats()["kernel_ms"]
        return median_of(run, a.reps)

    # the shipped choice, and the scale
    ctx, p = context()
    for spp in (0, 2):
        q = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT)

        def feat():
            ctx.render_features_device(q, d_guides.data_ptr(), d_guides.numel())
            return ctx.trace_stats()["kernel_ms"]
        ms, ts = median_of(feat, a.reps)
        emit({"case": "scale", "what": "render_features_device", "spp": spp, "us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})

    def frame():
        ctx.accum_frame_device(p, d_img.data_ptr())
        return ctx.stats()["kernel_ms"]
    ms, ts = median_of(frame, a.reps)
    emit({"case": "scale", "what": "accum_frame_device", "spp": 2, "us": round(ms * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})
    for source in ("accum", "adapt"):
        for levels in (3, 5):
            for f32 in (False, True):
                ms, ts = denoise_ms(ctx, p, source, levels, f32)
                fl = floor_us(levels, source, f32)
                emit({"case": "denoise", "source": source, "levels": levels, "out": "f32" if f32 else "rgba8", "us": round(ms * 1e3, 1), "all_ms": ts,
                      "floor_us": round(fl, 1), "times_floor": round(ms * 1e3 / fl, 2), "kernel": ctx.last_kernel()})
    ctx.close()

    # per level: all direct, and only the last level staged
    direct = {0: 0.0}
    ctx, p = context(0)
    q = m.make_params(W, H, 2, mode=m.MIRT_MODE_PT)
    ctx.render_features_device(q, d_guides.data_ptr(), d_guides.numel())
    ctx.accum_frame_device(p, d_img.data_ptr())
    for levels in range(1, a.max_level + 1):
        ms, ts = denoise_ms(ctx, p, "accum", levels, False)
        direct[levels] = ms
        emit({"case": "level", "shape": "direct", "level": levels - 1, "step": 1 << (levels - 1), "levels": levels, "us": round(ms * 1e3, 1),
              "added_us": round((ms - direct[levels - 1]) * 1e3, 1), "all_ms": ts, "kernel": ctx.last_kernel()})
    ctx.close()
    for levels in range(1, a.max_level + 1):
        ctx, p = context(1 << (levels - 1))
        ctx.accum_frame_device(p, d_img.data_ptr())
        ms, ts = denoise_ms(ctx, p, "accum", levels, False)
        emit({"case": "level", "shape": "staged", "level": levels - 1, "step": 1 << (levels - 1), "levels": levels, "us": round(ms * 1e3, 1),
              "added_us": round((ms - direct[levels - 1]) * 1e3, 1), "staged_minus_direct_us": round((ms - direct[levels]) * 1e3, 1), "all_ms": ts,
              "kernel": ctx.last_kernel()})
        ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
