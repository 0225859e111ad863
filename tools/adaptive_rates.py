#!/usr/bin/env python3
"""Adaptive-sampling rates (mirt_ctx_adapt_*): one JSON line per case, APPENDED to
profiles/r16_adaptive_rates.jsonl (profiles/r17_adaptive_pool_rates.jsonl with --pool) and printed.

Worlds: the RTIOW-style fields of tests/hbm_worlds.py at 484 and at 1 M spheres (--spheres), set with MIRT_SCENE_HBM, the tree built
on the device, seen at 1920 x 1080 with 8 bounces.  Cases (--cases, any of a,b,c), every one in alternating windows in ONE process,
the median of --reps windows after a warm-up of each variant, every window's figure beside it:
  a  adaptive against uniform.  `uniform`: mirt_ctx_accum_add of --max-spp samples in one launch (what the library offered before).
     `adaptive_<tolerance>`: mirt_ctx_adapt_step_device in steps of --step until a step lists nothing (the host reads the count after
     every step, as Raytracer.render_adaptive does), min_samples = the step, max_samples = --max-spp, for every --tolerances entry.
     A window is ONE such run from cleared records, host clock around it, ending in a synchronise; the resets are outside.  Reported:
     time, samples taken, and both as ratios to uniform; for the adaptive runs also the sum of the steps' own device times.
  b  the price of the machinery: tolerance 0 and min = max = --machinery-spp, so every pixel is in every step, against mirt_ctx_accum_add
     of the same samples in the same steps.  Windows of untimed launches back to back between two device events on one torch stream.
     The sums are compared once.  (The split into select and render comes from a kernel trace, a run of its own: --fold-trace.)
  c  mirt_ctx_adapt_resolve_device against resolve_accum_kernel (mirt_ctx_accum_frame_device with spp = 0), the same kind of windows.
  e  the empty step (--pool only): the records of a finished run, so that a step lists nothing and its render launch is a grid of blocks
     that return at once -- the whole step (select, scan, compact, render) with and without MIRT_ADAPT_POOL, windows as in c.
  r  (--run) the adaptive RUN, mirt_ctx_adapt_run_device: one call queues max_spp / step + 1 steps and the host waits
     once.  Per --tolerances entry, in alternating windows like case a: `uniform`; `loop_pool`, the host-driven pooled loop of case a;
     `run_0`, the same steps as one run (min_items 0: nothing grows, only the host's reads are gone); `run_<min_items>_<cap>` for every
     --min-items entry (`auto`: half of, once and twice the paths the device keeps in flight, compute units x the plan's waves x slots)
     and every --caps entry, with the samples each takes beside its time (growth spends samples) and its log.  All with MIRT_ADAPT_POOL.
     `tail`: the records of a converged run, then a run of 32 steps that all list nothing -- the price of the steps behind the empty
     one, pooled and unpooled, per step.  Lines go to profiles/r18_adaptive_run_rates.jsonl.
  l  (--lds) the world once as a scene in LDS and once as a MIRT_SCENE_HBM scene, two contexts in ONE process, per
     --tolerances entry in alternating windows like case a: `uniform_lds`, mirt_ctx_accum_add of --max-spp samples on the LDS scene with
     its default schedule; `lds_loop`, the host-driven loop with MIRT_ADAPT_LDS; `lds_run_0` and `lds_run_<min_items>_<cap>`, runs with it
     (--min-items / --caps: one pair, 10.14's best grown parameters by default); `hbm_loop_pool`, `hbm_run_0`, `hbm_run_<min_items>_<cap>`,
     the same on the HBM scene with MIRT_ADAPT_POOL.  The records of every LDS variant are compared with its HBM twin's once.
  m  (--lds) the price of the machinery on the LDS scene: tolerance 0 and min = max = --machinery-spp, every pixel in every step, with
     MIRT_ADAPT_LDS against mirt_ctx_accum_add of the same samples in the same steps on the same context; windows as in b.
     Lines go to profiles/r20_adaptive_lds_rates.jsonl.
--pool     adds the twin of every adaptive variant with MIRT_ADAPT_POOL (a: adaptive_<tolerance>_pool, b: adapt_pool) in
           the same alternating windows, compares their records with the unpooled variant's, and enables case e.
--fold-trace FILE   no device: reads the *_kernel_trace.csv of a rocprofv3 --kernel-trace --stats run and appends one line with the calls
                    and the median time of every adapt_*, render_pt_hbm* and resolve_accum kernel in it.

Run every world and case as a process of its own under its own time limit, e.g.
  timeout -k 10 300 python tools/adaptive_rates.py --spheres 484 --cases a
usage: python tools/adaptive_rates.py [--pool] [--run] [--lds] [--min-items auto] [--caps 32,64] [--spheres 484,1000000] [--cases a,b,c,e] [--reps 5] [--max-spp 256] [--step 8] [--tolerances 4096,1024]
                                      [--machinery-spp 32] [--window-ms 200] [--out profiles/r16_adaptive_rates.jsonl] [--fold-trace FILE]"""
from __future__ import annotations

import argparse
import csv
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

W, H = 1920, 1080
BOUNCES = 8


def fold_trace(path: str) -> dict:
    durations = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "adapt_" in name or "render_pt_" in name or "resolve_accum" in name:
                short = name.replace("mirt::exact_build::", "").replace("void ", "").split("(")[0]
                durations.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {"case": "kernel_trace", "source": Path(path).name,
            "kernels": {k: {"calls": len(v), "median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                        for k, v in durations.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spheres", default="484,1000000")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--step", type=int, default=8)
    ap.add_argument("--tolerances", default="4096,1024")
    ap.add_argument("--machinery-spp", type=int, default=32)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--pool", action="store_true", help="also time every adaptive variant with MIRT_ADAPT_POOL")
    ap.add_argument("--run", action="store_true", help="case r: adaptive runs (mirt_ctx_adapt_run_device) against the host-driven loop")
    ap.add_argument("--lds", action="store_true", help="cases l, m: MIRT_ADAPT_LDS on the world held in LDS against the HBM builds and against uniform sampling in LDS")
    ap.add_argument("--min-items", default="auto")
    ap.add_argument("--caps", default="32,64")
    ap.add_argument("--out", default="")
    ap.add_argument("--fold-trace", default="")
    ap.add_argument("--note", default="", help="copied into every line")
    a = ap.parse_args()
    if a.run:
        a.cases = "r"
    if a.lds:
        a.cases = a.cases if set(a.cases.split(",")) <= {"l", "m"} else "l,m"
        a.spheres = "484" if a.spheres == "484,1000000" else a.spheres       # the world must fit LDS
        a.min_items = "917504" if a.min_items == "auto" else a.min_items     # 10.14's best grown run on this world
        a.caps = "32" if a.caps == "32,64" else a.caps
    if not a.out:
        a.out = str(ROOT / "profiles" / ("r20_adaptive_lds_rates.jsonl" if a.lds else "r18_adaptive_run_rates.jsonl" if a.run else "r17_adaptive_pool_rates.jsonl" if a.pool else "r16_adaptive_rates.jsonl"))

    def emit(line):
        if a.note:
            line["note"] = a.note
        print(json.dumps(line), flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    if a.fold_trace:
        emit(fold_trace(a.fold_trace))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("adaptive_rates.py measures on the GPU: no device visible")
    import weekend_raytracer_wgpu_amd as m
    from hbm_worlds import look, rtiow_field, scene_from_arrays
    npix = W * H
    cases = [c for c in a.cases.split(",") if c]
    stream = torch.cuda.Stream(device="cuda:0")
    d_img = torch.zeros(4 * npix, dtype=torch.uint8, device="cuda:0")

    def window(fn, count):
        """`count` calls back to back between two device events on the torch stream -> ms per call."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(count):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / count

    for n in [int(x) for x in a.spheres.split(",") if x]:
        arr, mats, tex = rtiow_field(n, seed=n)
        eye = (13, 2, 3) if n < 5000 else (40, 6, 30)                 # the views of tools/radiance_rates.py
        sd = scene_from_arrays(look(W, H, eye, (0, 0, 0), vfov=25 if n < 5000 else 35), arr, mats, tex)
        ctx = m.Context(0)
        ctx.set_scene(sd, hbm=True, bvh="device")
        base = {"world": f"rtiow_field({n})", "n_spheres": n, "max_depth": ctx.bvh_info()["plan"]["max_depth"], "width": W, "height": H,
                "num_bounces": BOUNCES, "reps": a.reps}
        pt = lambda spp: m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=BOUNCES)

        if "l" in cases or "m" in cases:
            lds_ctx = m.Context(0)
            lds_ctx.set_scene(sd)                                       # the same world, in LDS

        if "l" in cases:
            p_step, p_all = pt(a.step), pt(a.max_spp)
            max_steps = a.max_spp // a.step + 1
            items, cap = int(a.min_items.split(",")[0]), int(a.caps.split(",")[0])

            def uniform_lds():
                lds_ctx.accum_reset(p_all)
                lds_ctx.synchronize()
                t0 = time.perf_counter()
                lds_ctx.accum_add(p_all)
                lds_ctx.synchronize()
                return {"ms": (time.perf_counter() - t0) * 1e3, "samples": npix * a.max_spp, "kernel": lds_ctx.last_kernel()}

            def loop_on(c, adapt):
                c.adapt_reset(p_step)
                c.synchronize()
                t0 = time.perf_counter()
                while True:
                    c.adapt_step(p_step, adapt)
                    st = c.adapt_stats()                                # waits for the step: the host must know whether to go on
                    if st["active"] == 0:
                        break
                return {"ms": (time.perf_counter() - t0) * 1e3, "samples": st["total_samples"], "steps": st["steps"], "kernel": c.last_kernel()}

            def run_on(c, adapt, min_items, max_spp):
                c.adapt_reset(p_step)
                c.synchronize()
                t0 = time.perf_counter()
                c.adapt_run(p_step, adapt, m.make_adapt_run(max_steps, min_items, max_spp))
                st = c.adapt_stats()                                    # the one wait
                ms = (time.perf_counter() - t0) * 1e3
                log = c.adapt_run_log()
                return {"ms": ms, "samples": st["total_samples"], "steps": int((log[:, 0] != 0).sum()), "device_ms": st["kernel_ms"], "active": st["active"],
                        "log": log[log[:, 0] != 0].tolist(), "kernel": c.last_kernel()}

            for tol in [int(x) for x in a.tolerances.split(",") if x]:
                on_lds = m.make_adapt_params(a.step, a.max_spp, tol, lds=True)
                on_hbm = m.make_adapt_params(a.step, a.max_spp, tol, pool=True)
                grown = f"run_{items}_{cap}"
                runs = {"uniform_lds": (None, uniform_lds),
                        "lds_loop": (lds_ctx, lambda: loop_on(lds_ctx, on_lds)), "hbm_loop_pool": (ctx, lambda: loop_on(ctx, on_hbm)),
                        "lds_run_0": (lds_ctx, lambda: run_on(lds_ctx, on_lds, 0, 0)), "hbm_run_0": (ctx, lambda: run_on(ctx, on_hbm, 0, 0)),
                        "lds_" + grown: (lds_ctx, lambda: run_on(lds_ctx, on_lds, items, cap)), "hbm_" + grown: (ctx, lambda: run_on(ctx, on_hbm, items, cap))}
                last, recs = {}, {}
                for k, (c, fn) in runs.items():                         # warm-up; the records of every adaptive variant, once
                    last[k] = fn()
                    if c is not None:
                        recs[k] = c.adapt_read()
                same = {k: bool(np.array_equal(recs[k].view(np.uint8), recs[("hbm_loop_pool" if k == "lds_loop" else "hbm" + k[3:])].view(np.uint8)))
                        for k in recs if k.startswith("lds_")}
                assert all(same.values()), same                         # the contract: the same bytes in LDS and in HBM
                t = {k: [] for k in runs}
                for _ in range(a.reps):
                    for k, (_, fn) in runs.items():
                        last[k] = fn()
                        assert last[k].get("active", 0) == 0, (k, last[k])      # every run converged within max_steps
                        t[k].append(last[k]["ms"])
                med = {k: statistics.median(v) for k, v in t.items()}
                emit({**base, "case": "l_adaptive_lds", "tolerance": tol, "max_spp": a.max_spp, "step": a.step, "min_samples": a.step, "max_steps": max_steps,
                      "ms": {k: round(v, 2) for k, v in med.items()}, "spread_ms": {k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
                      "samples": {k: int(last[k]["samples"]) for k in runs},
                      "time_over_uniform_lds": {k: round(med[k] / med["uniform_lds"], 3) for k in runs},
                      "lds_over_hbm": {k: round(med[k] / med["hbm_loop_pool" if k == "lds_loop" else "hbm" + k[3:]], 3) for k in runs if k.startswith("lds_")},
                      "samples_over_uniform": {k: round(last[k]["samples"] / last["uniform_lds"]["samples"], 4) for k in runs},
                      "sampling_steps": {k: last[k]["steps"] for k in runs if "steps" in last[k]},
                      "device_ms_of_the_run": {k: round(last[k]["device_ms"], 2) for k in runs if "device_ms" in last[k]},
                      "lds_records_equal_hbm": same, "logs": {k: last[k]["log"] for k in runs if last[k].get("log")},
                      "kernels": {k: last[k]["kernel"] for k in runs}, "all_ms": {k: [round(x, 2) for x in v] for k, v in t.items()}})

        if "m" in cases:
            n_steps = a.machinery_spp // a.step
            p_step = pt(a.step)
            adapt = m.make_adapt_params(a.machinery_spp, a.machinery_spp, 0, lds=True)

            def run_adapt_lds():
                for _ in range(n_steps):
                    lds_ctx.adapt_step(p_step, adapt, stream=stream.cuda_stream)

            def run_accum_lds():
                for _ in range(n_steps):
                    lds_ctx.accum_add(p_step, stream=stream.cuda_stream)

            lds_ctx.adapt_reset(p_step)
            lds_ctx.accum_reset(p_step)
            run_adapt_lds()
            kernels = {"adapt_lds": lds_ctx.last_kernel()}
            run_accum_lds()
            kernels["accum_lds"] = lds_ctx.last_kernel()
            torch.cuda.synchronize()
            same = bool(np.array_equal(lds_ctx.adapt_read()["sum"], lds_ctx.accum_read(p_step).reshape(-1, 3)))
            lds_ctx.set_timing(False)

            def fresh_lds(fn, reset):
                reset(p_step)
                torch.cuda.synchronize()
                return window(fn, 1)

            variants = {"adapt_lds": (run_adapt_lds, lds_ctx.adapt_reset), "accum_lds": (run_accum_lds, lds_ctx.accum_reset)}
            for fn, reset in variants.values():
                fresh_lds(fn, reset)
            t = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, (fn, reset) in variants.items():
                    t[k].append(fresh_lds(fn, reset))
            lds_ctx.set_timing(True)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({**base, "case": "m_price_of_the_machinery_lds", "samples_per_pixel": a.machinery_spp, "step": a.step, "steps": n_steps,
                  "ms": {k: round(v, 3) for k, v in med.items()}, "adapt_over_accum": round(med["adapt_lds"] / med["accum_lds"], 3), "same_sums": same,
                  "kernels": kernels, "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}})

        if "l" in cases or "m" in cases:
            lds_ctx.close()

        if "a" in cases:
            p_step, p_all = pt(a.step), pt(a.max_spp)

            def uniform():
                ctx.accum_reset(p_all)
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.accum_add(p_all)
                ctx.synchronize()
                return {"ms": (time.perf_counter() - t0) * 1e3, "samples": npix * a.max_spp, "kernel": ctx.last_kernel()}

            def adaptive(tol, pool=False):
                adapt = m.make_adapt_params(a.step, a.max_spp, tol, pool)
                ctx.adapt_reset(p_step)
                ctx.synchronize()
                device_ms, active = 0.0, []
                t0 = time.perf_counter()
                while True:
                    ctx.adapt_step(p_step, adapt)
                    st = ctx.adapt_stats()                          # waits for the step: the host must know whether to go on
                    device_ms += st["kernel_ms"]
                    active.append(st["active"])
                    if st["active"] == 0:
                        break
                ms = (time.perf_counter() - t0) * 1e3
                return {"ms": ms, "samples": st["total_samples"], "steps": st["steps"], "device_ms": device_ms, "active": active, "kernel": ctx.last_kernel()}

            runs = {"uniform": uniform}
            for tol in [int(x) for x in a.tolerances.split(",") if x]:
                runs[f"adaptive_{tol}"] = lambda tol=tol: adaptive(tol)
                if a.pool:
                    runs[f"adaptive_{tol}_pool"] = lambda tol=tol: adaptive(tol, True)
            last, recs = {}, {}
            for k, fn in runs.items():                                 # warm-up; the records of every adaptive variant, once
                last[k] = fn()
                if k != "uniform":
                    recs[k] = ctx.adapt_read()
            same = {k: bool(np.array_equal(recs[k].view(np.uint8), recs[k[:-5]].view(np.uint8))) for k in recs if k.endswith("_pool")}
            t = {k: [] for k in runs}
            for _ in range(a.reps):
                for k, fn in runs.items():
                    last[k] = fn()
                    t[k].append(last[k]["ms"])
            med = {k: statistics.median(v) for k, v in t.items()}
            counts = ctx.adapt_read()["samples"]                        # of the last adaptive run
            emit({**base, "case": "a_adaptive_against_uniform", "max_spp": a.max_spp, "step": a.step, "min_samples": a.step,
                  "ms": {k: round(v, 2) for k, v in med.items()}, "samples": {k: int(last[k]["samples"]) for k in runs},
                  "time_over_uniform": {k: round(med[k] / med["uniform"], 3) for k in runs},
                  "samples_over_uniform": {k: round(last[k]["samples"] / last["uniform"]["samples"], 4) for k in runs},
                  "steps": {k: last[k]["steps"] for k in runs if "steps" in last[k]},
                  "device_ms_of_the_steps": {k: round(last[k]["device_ms"], 2) for k in runs if "device_ms" in last[k]},
                  "active_per_step": {k: last[k]["active"] for k in runs if "active" in last[k]},
                  "last_run_pixels_at_max": int((counts >= a.max_spp).sum()), "last_run_median_samples": int(np.median(counts)),
                  **({"pooled_records_equal": same, "time_over_unpooled": {k: round(med[k] / med[k[:-5]], 3) for k in same}} if a.pool else {}),
                  "kernels": {k: last[k]["kernel"] for k in runs}, "all_ms": {k: [round(x, 2) for x in v] for k, v in t.items()}})

        if "r" in cases:
            p_step, p_all = pt(a.step), pt(a.max_spp)
            max_steps = a.max_spp // a.step + 1
            plan = m.adapt_pool_plan(base["max_depth"])
            in_flight = torch.cuda.get_device_properties(0).multi_processor_count * plan["waves_per_cu"] * plan["slots"]
            min_items = [in_flight // 2, in_flight, 2 * in_flight] if a.min_items == "auto" else [int(x) for x in a.min_items.split(",") if x]
            caps = [int(x) for x in a.caps.split(",") if x]

            def uniform():
                ctx.accum_reset(p_all)
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.accum_add(p_all)
                ctx.synchronize()
                return {"ms": (time.perf_counter() - t0) * 1e3, "samples": npix * a.max_spp, "kernel": ctx.last_kernel()}

            def loop(tol):
                adapt = m.make_adapt_params(a.step, a.max_spp, tol, True)
                ctx.adapt_reset(p_step)
                ctx.synchronize()
                t0 = time.perf_counter()
                while True:
                    ctx.adapt_step(p_step, adapt)
                    st = ctx.adapt_stats()                          # waits for the step: the host must know whether to go on
                    if st["active"] == 0:
                        break
                return {"ms": (time.perf_counter() - t0) * 1e3, "samples": st["total_samples"], "steps": st["steps"], "kernel": ctx.last_kernel()}

            def one_run(tol, items, cap, steps=max_steps, pool=True, reset=True):
                adapt, run = m.make_adapt_params(a.step, a.max_spp, tol, pool), m.make_adapt_run(steps, items, cap)
                if reset:
                    ctx.adapt_reset(p_step)
                ctx.synchronize()
                before = ctx.adapt_stats()["total_samples"]
                t0 = time.perf_counter()
                ctx.adapt_run(p_step, adapt, run)
                st = ctx.adapt_stats()                              # the one wait
                ms = (time.perf_counter() - t0) * 1e3
                log = ctx.adapt_run_log()
                return {"ms": ms, "samples": st["total_samples"] - before, "steps": int((log[:, 0] != 0).sum()), "device_ms": st["kernel_ms"], "active": st["active"],
                        "log": log[log[:, 0] != 0].tolist(), "kernel": ctx.last_kernel()}

            for tol in [int(x) for x in a.tolerances.split(",") if x]:
                runs = {"uniform": uniform, "loop_pool": lambda: loop(tol), "run_0": lambda: one_run(tol, 0, 0)}
                for cap in caps:
                    for items in min_items:
                        runs[f"run_{items}_{cap}"] = lambda items=items, cap=cap: one_run(tol, items, cap)
                # the tail: behind run_0's converged records, 32 steps that list nothing
                runs["tail32_pool"] = lambda: one_run(tol, 0, 0, 32, True, False)
                runs["tail32_plain"] = lambda: one_run(tol, 0, 0, 32, False, False)
                last, recs = {}, {}
                for k, fn in runs.items():                             # warm-up; the records of the loop and of the run that repeats it
                    if k.startswith("tail"):
                        one_run(tol, 0, 0)
                    last[k] = fn()
                    if k in ("loop_pool", "run_0"):
                        recs[k] = ctx.adapt_read()
                same = bool(np.array_equal(recs["loop_pool"].view(np.uint8), recs["run_0"].view(np.uint8)))
                t = {k: [] for k in runs}
                for _ in range(a.reps):
                    for k, fn in runs.items():
                        if k.startswith("tail"):
                            one_run(tol, 0, 0)                         # converged records, outside the window
                        last[k] = fn()
                        assert last[k].get("active", 0) == 0, (k, last[k])      # every run converged within max_steps
                        t[k].append(last[k]["ms"])
                med = {k: statistics.median(v) for k, v in t.items()}
                assert last["tail32_pool"]["samples"] == 0 and last["tail32_plain"]["samples"] == 0
                emit({**base, "case": "r_adaptive_run", "tolerance": tol, "max_spp": a.max_spp, "step": a.step, "min_samples": a.step, "max_steps": max_steps,
                      "paths_in_flight": in_flight, "ms": {k: round(v, 2) for k, v in med.items()},
                      "spread_ms": {k: [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
                      "samples": {k: int(last[k]["samples"]) for k in runs}, "time_over_loop": {k: round(med[k] / med["loop_pool"], 3) for k in runs},
                      "time_over_uniform": {k: round(med[k] / med["uniform"], 3) for k in runs},
                      "samples_over_uniform": {k: round(last[k]["samples"] / last["uniform"]["samples"], 4) for k in runs},
                      "sampling_steps": {k: last[k]["steps"] for k in runs if "steps" in last[k]},
                      "device_ms_of_the_run": {k: round(last[k]["device_ms"], 2) for k in runs if "device_ms" in last[k]},
                      "us_per_empty_step": {k: round(med[k] / 32 * 1e3, 1) for k in runs if k.startswith("tail")},
                      "run_0_records_equal_the_loops": same, "logs": {k: last[k]["log"] for k in runs if last[k].get("log")},
                      "kernels": {k: last[k]["kernel"] for k in runs}, "all_ms": {k: [round(x, 2) for x in v] for k, v in t.items()}})

        if "b" in cases:
            n_steps = a.machinery_spp // a.step
            p_step = pt(a.step)
            adapt = m.make_adapt_params(a.machinery_spp, a.machinery_spp, 0)

            def run_adapt():
                for _ in range(n_steps):
                    ctx.adapt_step(p_step, adapt, stream=stream.cuda_stream)

            adapt_pool = m.make_adapt_params(a.machinery_spp, a.machinery_spp, 0, True)

            def run_adapt_pool():
                for _ in range(n_steps):
                    ctx.adapt_step(p_step, adapt_pool, stream=stream.cuda_stream)

            def run_accum():
                for _ in range(n_steps):
                    ctx.accum_add(p_step, stream=stream.cuda_stream)

            # the same sums, once (timing on: the launches carry their events)
            ctx.adapt_reset(p_step)
            ctx.accum_reset(p_step)
            run_adapt()
            run_accum()
            torch.cuda.synchronize()
            same = bool(np.array_equal(ctx.adapt_read()["sum"], ctx.accum_read(p_step).reshape(-1, 3)))
            kernels = {}
            same_pool = None
            if a.pool:
                plain = ctx.adapt_read()
                ctx.adapt_reset(p_step)
                run_adapt_pool()
                torch.cuda.synchronize()
                kernels["adapt_pool"] = ctx.last_kernel()
                same_pool = bool(np.array_equal(ctx.adapt_read().view(np.uint8), plain.view(np.uint8)))
            ctx.adapt_step(p_step, adapt, stream=stream.cuda_stream)
            kernels["adapt"] = ctx.last_kernel()
            ctx.accum_add(p_step, stream=stream.cuda_stream)
            kernels["accum"] = ctx.last_kernel()
            torch.cuda.synchronize()
            ctx.set_timing(False)

            def fresh(fn, reset):
                """one window: cleared buffers (outside the events), then n_steps steps"""
                reset(p_step)
                torch.cuda.synchronize()
                return window(fn, 1)

            variants = {"adapt": (run_adapt, ctx.adapt_reset), "accum": (run_accum, ctx.accum_reset)}
            if a.pool:
                variants["adapt_pool"] = (run_adapt_pool, ctx.adapt_reset)
            for fn, reset in variants.values():
                fresh(fn, reset)
            t = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, (fn, reset) in variants.items():
                    t[k].append(fresh(fn, reset))
            ctx.set_timing(True)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({**base, "case": "b_price_of_the_machinery", "samples_per_pixel": a.machinery_spp, "step": a.step, "steps": n_steps,
                  "ms": {k: round(v, 3) for k, v in med.items()}, "adapt_over_accum": round(med["adapt"] / med["accum"], 3), "same_sums": same,
                  **({"pool_over_accum": round(med["adapt_pool"] / med["accum"], 3), "pool_over_adapt": round(med["adapt_pool"] / med["adapt"], 3),
                      "pooled_records_equal": same_pool} if a.pool else {}),
                  "kernels": kernels, "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}})

        if "c" in cases:
            p = pt(a.step)
            adapt = m.make_adapt_params(a.step, a.step, 0)
            ctx.adapt_reset(p)
            ctx.accum_reset(p)
            ctx.adapt_step(p, adapt)
            ctx.accum_add(p)
            ctx.synchronize()
            p0 = pt(0)
            launch = {"adapt_resolve": lambda: ctx.adapt_resolve_device(p, d_img.data_ptr(), stream=stream.cuda_stream),
                      "accum_resolve": lambda: ctx.accum_frame_device(p0, d_img.data_ptr(), stream=stream.cuda_stream)}
            img = {}
            ctx.set_timing(False)
            counts = {}
            for k, fn in launch.items():
                window(fn, 1)
                img[k] = d_img.cpu().numpy().copy()
                counts[k] = max(1, int(round(a.window_ms / max(window(fn, 4), 1e-3))))
                window(fn, counts[k])
            t = {k: [] for k in launch}
            for _ in range(a.reps):
                for k, fn in launch.items():
                    t[k].append(window(fn, counts[k]))
            ctx.set_timing(True)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({**base, "case": "c_resolve", "us": {k: round(v * 1e3, 1) for k, v in med.items()},
                  "adapt_over_accum": round(med["adapt_resolve"] / med["accum_resolve"], 3), "same_image": bool(np.array_equal(img["adapt_resolve"], img["accum_resolve"])),
                  "bytes_read_per_pixel": {"adapt_resolve": 48, "accum_resolve": 24}, "launches_per_window": counts,
                  "all_us": {k: [round(x * 1e3, 1) for x in v] for k, v in t.items()}})
        if "e" in cases and a.pool:
            p = pt(a.step)
            done = m.make_adapt_params(a.step, a.step, 0)
            ctx.adapt_reset(p)
            ctx.adapt_step(p, done)                                     # every pixel holds min = max samples: the next step lists nothing
            ctx.synchronize()
            launch, kernels = {}, {}
            for k, pool in (("empty_step", False), ("empty_step_pool", True)):
                ad = m.make_adapt_params(a.step, a.step, 0, pool)
                launch[k] = lambda ad=ad: ctx.adapt_step(p, ad, stream=stream.cuda_stream)
                launch[k]()
                torch.cuda.synchronize()
                assert ctx.adapt_stats()["active"] == 0
                kernels[k] = ctx.last_kernel()
            ctx.set_timing(False)
            counts = {}
            for k, fn in launch.items():
                window(fn, 1)
                counts[k] = max(1, int(round(a.window_ms / max(window(fn, 4), 1e-3))))
                window(fn, counts[k])
            t = {k: [] for k in launch}
            for _ in range(a.reps):
                for k, fn in launch.items():
                    t[k].append(window(fn, counts[k]))
            ctx.set_timing(True)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({**base, "case": "e_empty_step", "what": "select + scan + compact + a render launch whose every block returns at once",
                  "us": {k: round(v * 1e3, 1) for k, v in med.items()}, "pool_over_plain": round(med["empty_step_pool"] / med["empty_step"], 3),
                  "render_blocks": {"empty_step": (npix + 63) // 64, "empty_step_pool": ((npix + 15) // 16 + 3) // 4},
                  "kernels": kernels, "launches_per_window": counts, "all_us": {k: [round(x * 1e3, 1) for x in v] for k, v in t.items()}})
        ctx.close()


if __name__ == "__main__":
    main()
