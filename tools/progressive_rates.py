#!/usr/bin/env python3
"""Progressive-frame rates: what one DISPLAYED frame of the reference's render loop costs, one JSON line per case.

Cases: 1080p, the reference's main.rs scene and the three-sphere scene, 1 / 2 / 4 spp per frame (its UI's choices) and 32 spp (the
pooled kernel).  Steps (each a child process under its own timeout; the chain stops at the first that fails):

  ab      ONE process loads this build and, given --parent-lib, a build of the parent commit, and times on each, alternating window by
          window: `frame` (mirt_ctx_accum_frame_device, this build only), `add` (mirt_ctx_accum_add alone), `render`
          (mirt_ctx_render_device), and `two_step_wall` (accum_add + accum_resolve to the host, host clock: the parent's only way to
          show a progressive frame).  A window = --frames calls queued back to back on the context's stream between two device events,
          after a warm-up window; the figure is the median of --windows windows, all windows are kept.  This build is measured TWICE
          (two contexts, "build" and "build_again"): the difference between those is the spread of repeated identical runs.
  trace   rocprofv3 --kernel-trace --stats (no counters) around `--step workload` on the parent build: per case --frames frames of
          accum_add + accum_resolve; the kernel trace gives the add kernel and resolve_accum_kernel per case (median over the frames).
  node    MirtNodeStats and wall time per frame of a loopback 4-member progressive frame beside a one-shot mirt_node_render frame of
          the same spp, and beside one context (loopback: every member on one GPU, no speed-up to be had).

usage: python tools/progressive_rates.py [--parent-lib tools/_scratch/libs/libmirt_parent.so] [--out profiles/r06_progressive_rates.jsonl]
       (the parent build: tools/node_timing.py's docstring)
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

W, H = 1920, 1080
SCENES = ("main_rs_scene", "three_spheres")
SPPS = (1, 2, 4, 32)


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--step", choices=("all", "ab", "trace", "workload", "node"), default="all")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--lib", default=None, help="workload step: the library to run (default: this build)")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r06_progressive_rates.jsonl"))
    ap.add_argument("--trace-dir", default=str(ROOT / "tools" / "_scratch" / "progressive_trace"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per step")
    return ap.parse_args()


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


class Lib:
    """One build of libmirt.so with a context of its own, through ctypes (a parent build exports fewer symbols)."""

    def __init__(self, path, name):
        import weekend_raytracer_wgpu_amd as m
        from weekend_raytracer_wgpu_amd import _abi
        self.name = name
        self.lib = m.lib() if path is None else C.CDLL(str(Path(path).resolve()))
        if path is not None:
            _abi.bind(self.lib, {k: v for k, v in _abi.SYMBOLS.items() if hasattr(self.lib, k)})
        self.has_frame = hasattr(self.lib, "mirt_ctx_accum_frame_device")
        self.ctx = C.c_void_p()
        self.ok(self.lib.mirt_ctx_create(0, C.byref(self.ctx)))
        self.ok(self.lib.mirt_ctx_set_timing(self.ctx, 0))           # a host that queues frame after frame
        h = C.c_void_p()
        self.ok(self.lib.mirt_ctx_frame_stream(self.ctx, 0, C.byref(h)))
        self.stream = h.value

    def ok(self, rc):
        assert rc == 0, (self.name, rc, self.lib.mirt_last_error())

    def set_scene(self, sd):
        sc = sd.as_c()
        self.ok(self.lib.mirt_ctx_set_scene(self.ctx, C.byref(sc)))

    def reset(self, p):
        self.ok(self.lib.mirt_ctx_accum_reset(self.ctx, C.byref(p)))

    def frame(self, p, d_out, nbytes):
        self.ok(self.lib.mirt_ctx_accum_frame_device(self.ctx, C.byref(p), C.c_void_p(d_out), nbytes, None))

    def add(self, p):
        self.ok(self.lib.mirt_ctx_accum_add(self.ctx, C.byref(p), None))

    def render(self, p, d_out, nbytes):
        self.ok(self.lib.mirt_ctx_render_device(self.ctx, C.byref(p), C.c_void_p(d_out), nbytes, None))

    def resolve(self, p, host):
        self.ok(self.lib.mirt_ctx_accum_resolve(self.ctx, C.byref(p), host.ctypes.data_as(C.c_void_p), host.nbytes))

    def kernel(self):
        return self.lib.mirt_ctx_last_kernel(self.ctx).decode()

    def sync(self):
        self.ok(self.lib.mirt_ctx_synchronize(self.ctx))

    def close(self):
        self.lib.mirt_ctx_destroy(self.ctx)


def step_ab(a):
    import numpy as np
    import torch
    import weekend_raytracer_wgpu_amd as m
    from helpers import scene_data
    libs = [Lib(None, "build"), Lib(None, "build_again")]
    if a.parent_lib:
        libs.insert(1, Lib(a.parent_lib, "parent"))
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    host = np.empty((H, W, 4), dtype=np.uint8)
    streams = {lb.name: torch.cuda.ExternalStream(lb.stream) for lb in libs}

    def window(lb, call, p):
        """us per call: `frames` calls back to back on the context's stream between two device events."""
        lb.reset(p)
        st = streams[lb.name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.frames):
            call(lb, p)
        e1.record(st)
        e1.synchronize()
        lb.sync()
        return e0.elapsed_time(e1) * 1e3 / a.frames

    def wall_window(lb, p):
        lb.reset(p)
        frames = max(20, a.frames // 4)
        t0 = time.perf_counter()
        for _ in range(frames):
            lb.add(p)
            lb.resolve(p, host)
        return (time.perf_counter() - t0) * 1e6 / frames

    ops = {"frame": lambda lb, p: lb.frame(p, out.data_ptr(), out.numel()),
           "add": lambda lb, p: lb.add(p),
           "render": lambda lb, p: lb.render(p, out.data_ptr(), out.numel())}
    for scene in SCENES:
        sd = scene_data(scene, W, H)
        for lb in libs:
            lb.set_scene(sd)
        for spp in SPPS:
            p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
            rec = {"case": "ab", "scene": scene, "width": W, "height": H, "spp": spp, "frames_per_window": a.frames, "windows": a.windows,
                   "unit": "us per call (device events; two_step_wall: host clock)"}
            for op, call in ops.items():
                users = [lb for lb in libs if op != "frame" or lb.has_frame]
                for lb in users:
                    window(lb, call, p)                                # warm-up window
                rec.setdefault("kernel", {})[op] = libs[0].kernel()
                all_us = {lb.name: [] for lb in users}
                for _ in range(a.windows):                             # alternating: one window per build per round
                    for lb in users:
                        all_us[lb.name].append(window(lb, call, p))
                rec[op] = {n: {"median_us": round(statistics.median(v), 2), "all_us": [round(x, 2) for x in v]} for n, v in all_us.items()}
            wall = {lb.name: [] for lb in libs}
            for lb in libs:
                wall_window(lb, p)
            for _ in range(a.windows):
                for lb in libs:
                    wall[lb.name].append(wall_window(lb, p))
            rec["two_step_wall"] = {n: {"median_us": round(statistics.median(v), 1), "all_us": [round(x, 1) for x in v]} for n, v in wall.items()}
            emit(a, rec)
    for lb in libs:
        lb.close()


def step_workload(a):
    """What the trace step profiles: per case a warm-up frame, then --frames frames of accum_add + accum_resolve."""
    import numpy as np
    import weekend_raytracer_wgpu_amd as m
    from helpers import scene_data
    lb = Lib(a.lib, "traced")
    host = np.empty((H, W, 4), dtype=np.uint8)
    for scene in SCENES:
        lb.set_scene(scene_data(scene, W, H))
        for spp in SPPS:
            p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
            lb.reset(p)
            for _ in range(a.frames + 1):
                lb.add(p)
                lb.resolve(p, host)
    lb.close()


def step_trace(a):
    if not a.parent_lib:
        print("trace: no --parent-lib, skipped", flush=True)
        return
    cmd = ["timeout", "-k", "10", str(a.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace_dir, "--",
           sys.executable, __file__, "--step", "workload", "--lib", a.parent_lib, "--frames", str(a.frames)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    traces = sorted(glob.glob(os.path.join(a.trace_dir, "**", "*_kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    assert traces, "rocprofv3 left no kernel trace"
    rows = []
    with open(traces[-1], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "render_pt_" in name or "resolve_accum_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    per_case = 2 * (a.frames + 1)
    assert len(rows) == per_case * len(SCENES) * len(SPPS), (len(rows), per_case)
    k = 0
    for scene in SCENES:
        for spp in SPPS:
            mine = rows[k + 2:k + per_case]                            # (the warm-up frame dropped)
            k += per_case
            adds = [(e - s) / 1e3 for s, e, n in mine if "render_pt_" in n]
            resolves = [(e - s) / 1e3 for s, e, n in mine if "resolve_accum_kernel" in n]
            assert len(adds) == len(resolves) == a.frames
            emit(a, {"case": "parent_trace", "scene": scene, "width": W, "height": H, "spp": spp, "frames": a.frames,
                     "add_kernel": next(n for _, _, n in mine if "render_pt_" in n),
                     "add_kernel_us": round(statistics.median(adds), 2), "resolve_kernel_us": round(statistics.median(resolves), 2),
                     "sum_us": round(statistics.median(adds) + statistics.median(resolves), 2),
                     "add_min_max_us": [round(min(adds), 2), round(max(adds), 2)],
                     "resolve_min_max_us": [round(min(resolves), 2), round(max(resolves), 2)]})


def step_node(a):
    import weekend_raytracer_wgpu_amd as m
    from helpers import scene_data
    frames = max(20, a.frames // 4)
    sd = scene_data("main_rs_scene", W, H)

    def wall_us(call, reset):
        out = []
        for i in range(a.windows + 1):
            reset()
            t0 = time.perf_counter()
            for _ in range(frames):
                call()
            if i:
                out.append((time.perf_counter() - t0) * 1e6 / frames)
        return round(statistics.median(out), 1)

    for spp in (2, 32):
        p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=8)
        rec = {"case": "node", "scene": "main_rs_scene", "width": W, "height": H, "spp": spp, "members": 4, "transport": "loopback",
               "unit": "wall us per blocking frame (host clock), MirtNodeStats of the last frame"}
        with m.Node([0] * 4) as node, m.Context(0) as ctx:
            node.set_scene(sd)
            ctx.set_scene(sd)
            rec["node_accum_frame_wall_us"] = wall_us(lambda: node.accum_frame(p), lambda: node.accum_reset(p))
            rec["node_accum_frame_stats"] = node.stats()
            rec["node_render_wall_us"] = wall_us(lambda: node.render(p), lambda: None)
            rec["node_render_stats"] = node.stats()
            rec["ctx_accum_frame_wall_us"] = wall_us(lambda: ctx.accum_frame(p), lambda: ctx.accum_reset(p))
            rec["ctx_render_wall_us"] = wall_us(lambda: ctx.render(p), lambda: None)
        emit(a, rec)


def main():
    a = parse_args()
    if a.step == "all":
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        open(a.out, "w").close()
        for step in ("ab", "node", "trace"):                            # every GPU step under its own time limit; stop at the first failure
            cmd = ["timeout", "-k", "10", str(a.timeout + 30), sys.executable, __file__, "--step", step, "--frames", str(a.frames), "--windows", str(a.windows), "--out", a.out,
                   "--trace-dir", a.trace_dir, "--timeout", str(a.timeout)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
            r = subprocess.run(cmd)
            if r.returncode != 0:
                print(f"step {step} failed with status {r.returncode}: stopping", file=sys.stderr)
                sys.exit(r.returncode)
        return
    {"ab": step_ab, "trace": step_trace, "workload": step_workload, "node": step_node}[a.step](a)


if __name__ == "__main__":
    main()
