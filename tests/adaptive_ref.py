"""The judge of mirt_ctx_adapt_* (host-side data only; a helper like radiance_frames.py, not a conftest; nothing here runs a kernel of
the library).

Everything in the adaptive loop is integer, so it has ONE right answer: which pixels a step samples, and every sum.  The oracle's
render_pt_sums at spp = 1, sample_begin = s is every pixel's sample s (its sums are additive over sample_begin:
tests/test_radiance_frames_cpu.py, and test_adaptive_abi.py once more for this input); the rule of include/mirt.h is restated here in
Python's unlimited integers, and replay() runs the loop: lists, counts, sum, even, samples after every step."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE
import hbm_worlds
import oracle_binding as ob

FLOOR = 1 << 17                             # MIRT_ADAPT_FLOOR

# the input of the whole-loop test
W, H = 48, 32
N_SPHERES = 300
BOUNCES, SEED = 8, 7
SPP, MIN_SAMPLES, MAX_SAMPLES, TOLERANCE = 4, 4, 32, 4096
N_STEPS = 9                                 # eight steps that sample, and the ninth, which is empty


def rule_active(s, e, n, min_samples, max_samples, tolerance) -> bool:
    """include/mirt.h, in Python integers: s, e = the three sums and the three even sums, n = samples."""
    s, e, n = [int(v) for v in s], [int(v) for v in e], int(n)
    err = sum(abs(2 * e[k] - s[k]) for k in range(3))
    mean = sum(s)
    converged = n >= 2 and err * (1 << 16) <= int(tolerance) * (mean + n * FLOOR)
    return n < int(max_samples) and (n < int(min_samples) or not converged)


def record_active(rec, min_samples, max_samples, tolerance) -> bool:
    return rule_active(rec["sum"], rec["even"], rec["samples"], min_samples, max_samples, tolerance)


def camera(w=W, h=H):
    return hbm_worlds.look(w, h, (13, 2, 3), (0, 0, 0), vfov=25, aperture=0.05)


@functools.lru_cache(maxsize=None)
def _field():
    return hbm_worlds.rtiow_field(N_SPHERES)


def scene(sky=None, w=W, h=H):
    arr, mats, tex = _field()
    return hbm_worlds.scene_from_arrays(camera(w, h), arr, mats, tex, sky)


def params(spp=SPP, flags=0, w=W, h=H, seed=SEED, bounces=BOUNCES, **rows):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, num_bounces=bounces, seed=seed, flags=flags, **rows)


_frames = {}


def sample_frames(scene_data, p, n_samples, key) -> np.ndarray:
    """uint64 [n_samples, pixels, 3]: the oracle's one-sample frames 0 .. n_samples - 1 of the rows `p` selects (compact, row-major).
    `key` names the scene; computed once per (key, rows, seed, sky flag), read-only."""
    k = (key, p.width, p.height, p.num_bounces, p.seed, p.flags & _abi.MIRT_FLAG_SKY_HOSEK, p.row_begin, p.row_end, p.tile_rows, p.n_parts, p.part)
    have = _frames.get(k)
    if have is None or len(have) < n_samples:
        out = []
        for s in range(n_samples):
            q = m.make_params(p.width, p.height, 1, mode=m.MIRT_MODE_PT, num_bounces=p.num_bounces, seed=p.seed,
                              flags=p.flags & _abi.MIRT_FLAG_SKY_HOSEK, sample_begin=s, row_begin=p.row_begin, row_end=p.row_end,
                              tile_rows=p.tile_rows, n_parts=p.n_parts, part=p.part)
            out.append(ob.render_pt_sums(scene_data, q).reshape(-1, 3))
        have = np.stack(out)
        have.flags.writeable = False
        _frames[k] = have
    return have[:n_samples]


def replay(frames, spp, min_samples, max_samples, tolerance, n_steps, start=None) -> list:
    """The loop in Python integers over frames [samples, pixels, 3] -> one dict per step: "list" (uint32, ascending), "records"
    (ADAPT_PIXEL_DTYPE, the buffer AFTER the step) and "total" (samples added since the reset).  start: the records to begin with."""
    npix = frames.shape[1]
    recs = np.zeros(npix, ADAPT_PIXEL_DTYPE) if start is None else start.copy()
    steps, total = [], 0
    for _ in range(n_steps):
        active = [i for i in range(npix) if record_active(recs[i], min_samples, max_samples, tolerance)]
        for i in active:
            n = int(recs["samples"][i])
            for s in range(n, n + spp):
                recs["sum"][i] += frames[s, i]
                if s % 2 == 0:
                    recs["even"][i] += frames[s, i]
            recs["samples"][i] = n + spp
        total += len(active) * spp
        steps.append({"list": np.asarray(active, np.uint32), "records": recs.copy(), "total": total})
    return steps


@functools.lru_cache(maxsize=None)
def reference_loop() -> tuple:
    """The N_STEPS steps of the whole-loop input (BVH and NO_GRID builds compute the same thing: one reference).  The preconditions
    that make the input worth running are asserted on the reference itself, before anything is compared with it."""
    frames = sample_frames(scene(), params(), MAX_SAMPLES + SPP, "field300")
    steps = replay(frames, SPP, MIN_SAMPLES, MAX_SAMPLES, TOLERANCE, N_STEPS)
    final = steps[-1]["records"]["samples"]
    for n in range(MIN_SAMPLES, MAX_SAMPLES + 1, SPP):
        assert int((final == n).sum()) >= 16, f"only {int((final == n).sum())} pixels end at {n} samples"
    for k, st in enumerate(steps[1:-1], 1):
        assert len(st["list"]) % 64 != 0, f"step {k} lists {len(st['list'])} pixels: no partial last wave"
    assert len(steps[0]["list"]) == W * H and len(steps[-1]["list"]) == 0, "the first step takes every pixel, the ninth none"
    return tuple(steps)


def corner_records() -> tuple:
    """(records, cases): the corners of the rule and seeded records.  cases = (min_samples, max_samples, tolerance) sets under which
    the records are interesting; 128 records, so that they fill a 64 x 2 buffer."""
    big = (1 << 56) - 1
    rows = []

    def add(s, e, n):
        rows.append((tuple(s), tuple(e), n))

    for n in (0, 1, 2, 3, 4, 31, 32, 33):                           # n = 0, 1, 2 and around max_samples = 32
        add((n * 300000,) * 3, (n * 150000,) * 3, n)                # halves agree
        add((n * 300000,) * 3, (0, 0, 0), n)                        # all of it in the odd half
    add((big,) * 3, (0,) * 3, 16)                                   # sums at 2^56 - 1, even = 0 and even = sum
    add((big,) * 3, (big,) * 3, 16)
    add((0,) * 3, (0,) * 3, 8)                                      # black: e = 0, the floor alone on the right
    # e x 2^16 one below, at and one above tolerance x (m + n x FLOOR), under the case (2, 2^24, 1): n = 2, tolerance = 1, so the
    # right-hand side is m + 2^18.  2 x even is even, hence e = m (mod 2): the two odd borders take e = 9, the even one e = 8.
    for e_want, d in ((9, -1), (8, 0), (9, 1)):
        m_sum = e_want * (1 << 16) - 2 * FLOOR + d                 # right-hand side - left-hand side = d
        s0 = m_sum - 200000
        assert (s0 - e_want) % 2 == 0
        add((s0, 100000, 100000), ((s0 - e_want) // 2, 50000, 50000), 2)
    rng = np.random.default_rng(20)
    while len(rows) < 128:
        n = int(rng.integers(0, 40))
        s = [int(v) for v in rng.integers(0, 1 << 22, 3) * max(n, 1)]
        e = [int(v * f) for v, f in zip(s, rng.uniform(0.35, 0.65, 3))]
        add(s, e, n)
    recs = np.zeros(len(rows), ADAPT_PIXEL_DTYPE)
    for i, (s, e, n) in enumerate(rows):
        recs["sum"][i], recs["even"][i], recs["samples"][i] = s, e, n
    cases = ((4, 32, 4096), (4, 32, 0), (4, 32, 0xFFFFFFFF), (0, 32, 4096), (4, 16, 4096), (2, 1 << 24, 1), (4, 32, 65536))
    return recs, cases
