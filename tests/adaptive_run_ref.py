"""The judge of mirt_ctx_adapt_run_* (host-side data only; a helper like adaptive_ref.py, not a conftest; nothing here runs a kernel of
the library).

A run is a loop of adaptive steps whose sample counts the DEVICE chooses, by an integer rule, from the list it has just built.  All of
it is integer, so a run has one right answer: run_spp is the rule of include/mirt.h in Python's unlimited integers, and replay_run
runs the loop over the oracle's one-sample frames -- per step the list, the records and the counter, and the log {count, spp}."""
from __future__ import annotations

import functools

import numpy as np

from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
from adaptive_ref import sample_frames, record_active, scene, params
import adaptive_ref as ar

W, H = ar.W, ar.H
BASE, MIN_SAMPLES, MAX_SAMPLES, TOLERANCE = ar.SPP, ar.MIN_SAMPLES, ar.MAX_SAMPLES, ar.TOLERANCE
N_FRAMES = 48                               # samples 0 .. 47: a pixel at 28 that a step of 16 takes to 44

# (max_steps, min_items, max_spp) -> the log the CPU oracle and the replay give for the input of DESIGN.md 10.12 (rtiow_field(300),
# 48 x 32 through the lens, 8 bounces, seed 7, base 4, min 4, max 32, tolerance 4096)
RUNS = {
    "three sizes": ((8, 3000, 16), [(1536, 4), (731, 8), (540, 8), (401, 8), (299, 16), (0, 0), (0, 0), (0, 0)]),
    "the cap binds": ((6, 4096, 8), [(1536, 4), (731, 8), (540, 8), (401, 8), (299, 8), (0, 0)]),
    "k jumps by two": ((4, 6144, 16), [(1536, 4), (731, 16), (479, 16), (0, 0)]),
}


def run_spp(count, base, min_items, max_spp) -> int:
    """include/mirt.h, in Python integers: the samples a step that lists `count` pixels takes of each."""
    count, base, min_items, cap = int(count), int(base), int(min_items), int(max_spp) or int(base)
    if count == 0:
        return 0
    spp = base
    while count * spp < min_items and spp != cap:
        spp *= 2
        assert spp <= cap, (base, cap)      # cap = base << m
    return spp


def _run_fields(run) -> tuple:
    if isinstance(run, _abi.MirtAdaptRun):
        assert run.flags == 0
        return int(run.max_steps), int(run.min_items), int(run.max_spp)
    return tuple(int(v) for v in run)


def replay_run(frames, base, min_samples, max_samples, tolerance, run, start=None) -> dict:
    """The run in Python integers over frames [samples, pixels, 3] -> {"steps": one dict per step of the run -- "list" (uint32,
    ascending; None for a step behind an empty one, which leaves the device's list as it is), "records" (ADAPT_PIXEL_DTYPE, the buffer
    AFTER the step) and "total" (samples added since the reset) --, "log": uint32 [max_steps, 2], {count, spp}}.  run: a MirtAdaptRun
    or (max_steps, min_items, max_spp); start: the records to begin with."""
    max_steps, min_items, max_spp = _run_fields(run)
    npix = frames.shape[1]
    recs = np.zeros(npix, ADAPT_PIXEL_DTYPE) if start is None else start.copy()
    steps, log, total, seen_empty = [], [], 0, False
    for _ in range(max_steps):
        active = [i for i in range(npix) if record_active(recs[i], min_samples, max_samples, tolerance)]
        spp = run_spp(len(active), base, min_items, max_spp)
        for i in active:
            n = int(recs["samples"][i])
            assert n + spp <= len(frames), f"pixel {i} needs sample {n + spp - 1}: {len(frames)} frames given"
            for s in range(n, n + spp):
                recs["sum"][i] += frames[s, i]
                if s % 2 == 0:
                    recs["even"][i] += frames[s, i]
            recs["samples"][i] = n + spp
            recs["_pad0"][i], recs["_pad1"][i] = 0, 0
        total += len(active) * spp
        assert not (seen_empty and active), "a step behind an empty one lists pixels: the records did not change"
        steps.append({"list": None if seen_empty else np.asarray(active, np.uint32), "records": recs.copy(), "total": total})
        log.append((len(active), spp))
        seen_empty = seen_empty or not active
    return {"steps": steps, "log": np.asarray(log, np.uint32).reshape(-1, 2)}


def frames_of(sky=None, flags=0, n=N_FRAMES) -> np.ndarray:
    return sample_frames(scene(sky), params(flags=flags), n, "field300")


@functools.lru_cache(maxsize=None)
def reference_run(name) -> dict:
    """The run RUNS[name] on the whole-loop input (BVH, NO_GRID and pooled builds compute the same thing: one reference)."""
    reference_runs()
    return replay_run(frames_of(), BASE, MIN_SAMPLES, MAX_SAMPLES, TOLERANCE, RUNS[name][0])


@functools.lru_cache(maxsize=None)
def reference_runs() -> bool:
    """What makes the three runs worth running, asserted ON THE REFERENCE before anything is compared with it."""
    frames = frames_of()
    got = {name: replay_run(frames, BASE, MIN_SAMPLES, MAX_SAMPLES, TOLERANCE, run) for name, (run, _) in RUNS.items()}
    for name, (run, log) in RUNS.items():
        assert [tuple(int(v) for v in e) for e in got[name]["log"]] == log, (name, got[name]["log"].tolist())
    first, capped, jump = (got[k] for k in ("three sizes", "the cap binds", "k jumps by two"))
    assert first["steps"][-1]["total"] == 24304 and capped["steps"][-1]["total"] == 21912
    final = first["steps"][-1]["records"]["samples"]
    held = {int(n): int((final == n).sum()) for n in np.unique(final)}
    assert held == {4: 805, 12: 191, 20: 139, 28: 102, 44: 299}, held
    assert min(held.values()) >= 16                                             # at least 16 pixels hold every final count
    assert int(final.max()) - MAX_SAMPLES > BASE                                # 44: above max_samples by more than base -- no clamp, not the argument
    assert len({int(s) for _, s in first["log"] if s}) == 3                     # three distinct step sizes in one run
    (_, min_items, cap), log = RUNS["three sizes"]
    assert any(c * s >= min_items and s < cap and c * s // 2 < min_items and s > BASE for c, s in log if c)      # growth stopped by the product
    (_, min_items, cap), log = RUNS["the cap binds"]
    assert (401, 8) in log and 401 * 8 == 3208 < min_items and cap == 8         # growth stopped by the cap
    assert [s for _, s in RUNS["k jumps by two"][1][:2]] == [4, 16]               # k jumps by two
    for name, (run, log) in RUNS.items():
        sampling = [c for c, _ in log if c]
        assert all(c % 16 != 0 and c % 64 != 0 for c in sampling[1:]), (name, sampling)      # ragged units, a partial last wave
        assert log[-1] == (0, 0) and len(sampling) < run[0]                     # the run ends before max_steps
    return True
