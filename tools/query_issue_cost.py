#!/usr/bin/env python3
"""What it costs the host to issue a query launch: wall microseconds per call over back-to-back calls on one stream, timing off
(mirt_ctx_set_timing(ctx, 0)), for builds of libmirt.so run alternately, each measurement in a fresh process.  The kernels of the
measured calls do next to nothing (64 rays, 16x16 pixels, a converged adaptive buffer), so a change in the plumbing between the C ABI
and the dispatch shows (profiles/r23_query_plan.md).

    python tools/query_issue_cost.py [--calls 2000] [--repeat 4] [--out FILE.json] PARENT.so NEW.so     -> a table (and the figures as JSON)

Every measurement is a child process (this file with --child) under its own time limit; the chain stops at the first child that fails.
A library's mean passes when it lies inside the first library's own min-max range widened by that range's width on each side.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

ROWS = ("trace_rays 64", "render_features 16x16", "trace_radiance 64", "trace_radiance 64 pool", "adapt_step 16x16", "adapt_step 16x16 pool",
        "adapt_step 16x16 lds", "adapt_run 16x16 x 8 steps")


def child(lib_path, calls):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import numpy as np
    import torch
    import weekend_raytracer_wgpu_amd as m
    from weekend_raytracer_wgpu_amd import _lib
    from helpers import scene_data
    _lib.LIB_PATH = Path(lib_path).resolve()                 # before the first call binds the library
    w = h = 16
    sd = scene_data("rtiow_final", w, h)                     # 484 spheres: a tree for the HBM context, the grid layout for the LDS one
    hbm, lds = m.Context(0), m.Context(0)
    hbm.set_scene(sd, hbm=True)
    lds.set_scene(sd)
    n = 64
    d = np.tile(np.array([0.0, -0.2, -1.0], np.float32), (n, 1)) + np.linspace(-0.3, 0.3, n, dtype=np.float32)[:, None] * np.array([1, 0, 0], np.float32)
    rays = torch.from_numpy(m.make_rays(np.array([0.0, 1.0, 6.0], np.float32), d).view(np.uint8)).cuda()
    rrays = torch.from_numpy(m.make_radiance_rays(np.array([0.0, 1.0, 6.0], np.float32), d).view(np.uint8)).cuda()
    out = torch.zeros(max(n, w * h) * 32, dtype=torch.uint8, device="cuda")
    p = m.make_params(w, h, 2, mode=m.MIRT_MODE_PT, num_bounces=8)
    run = m.make_adapt_run(8)
    # max_samples = 0: no pixel of the cleared buffer is active -- every step lists nothing and its render blocks return at once
    plain, pool, in_lds = (m.make_adapt_params(0, 0, 0, **kw) for kw in ({}, {"pool": True}, {"lds": True}))
    for c in (hbm, lds):
        c.set_timing(False)
        c.adapt_reset(p)
    calls_of = {
        ROWS[0]: (hbm, lambda: hbm.trace_rays_device(rays.data_ptr(), n, out.data_ptr())),
        ROWS[1]: (hbm, lambda: hbm.render_features_device(p, out.data_ptr(), out.numel())),
        ROWS[2]: (hbm, lambda: hbm.trace_radiance_device(rrays.data_ptr(), n, out.data_ptr(), 2)),
        ROWS[3]: (hbm, lambda: hbm.trace_radiance_device(rrays.data_ptr(), n, out.data_ptr(), 2, pool=True)),
        ROWS[4]: (hbm, lambda: hbm.adapt_step(p, plain)),
        ROWS[5]: (hbm, lambda: hbm.adapt_step(p, pool)),
        ROWS[6]: (lds, lambda: lds.adapt_step(p, in_lds)),
        ROWS[7]: (hbm, lambda: hbm.adapt_run(p, plain, run)),
    }
    res = {}
    for row, (ctx, call) in calls_of.items():
        for _ in range(50):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        t = time.perf_counter() - t0
        torch.cuda.synchronize()
        res[row] = {"us_per_call": round(1e6 * t / calls, 3), "kernel": ctx.last_kernel()}
    for c in (hbm, lds):
        c.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--out", help="also write the figures to this JSON file")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    if a.child:
        return child(a.libs[0], a.calls)
    runs = {lib: [] for lib in a.libs}
    for _ in range(a.repeat):
        for lib in a.libs:                                   # alternating, each a fresh process under its own time limit
            r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, __file__, "--child", "--calls", str(a.calls), lib], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"{lib}: the measuring process ended with {r.returncode}; nothing further is started\n{r.stderr[-2000:]}")
            runs[lib].append(json.loads(r.stdout.splitlines()[-1]))
    base, ok = a.libs[0], True
    table = {}
    for row in ROWS:
        table[row] = {lib: [x[row]["us_per_call"] for x in runs[lib]] for lib in a.libs}
        lo, hi = min(table[row][base]), max(table[row][base])
        print(f"{row:28s} {runs[base][0][row]['kernel']}")
        for lib in a.libs:
            v = table[row][lib]
            mean = sum(v) / len(v)
            inside = lo - (hi - lo) <= mean <= hi + (hi - lo)
            ok = ok and inside
            print(f"    {Path(lib).parent.parent.parent.name + '/' + Path(lib).name:32s} {' '.join(f'{x:8.2f}' for x in v)}   mean {mean:8.3f}"
                  + ("" if lib == base else f"   {'inside' if inside else 'OUTSIDE'} [{lo - (hi - lo):.2f}, {hi + (hi - lo):.2f}]"))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"calls": a.calls, "us_per_call": table}, indent=1) + "\n")
    print("every mean lies inside the first library's widened range" if ok else "a mean lies OUTSIDE the first library's widened range")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
