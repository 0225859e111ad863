"""The device's resolve (csrc/mirt_device_resolve.h: resolve_channel, exact build) against the oracle's
(om_resolve_channel), for sample counts on both of the device's routes (a power of two scales the sum with ldexp, any
other count divides, as the oracle always does) and all four combinations of MIRT_FLAG_NO_TONEMAP / MIRT_FLAG_NO_SRGB.

n <= 8: every sum of [0, n * (2^32 - 256)] is compared on the device (mprobe_resolve_sweep).  Larger n: every threshold
of the 255 codes (found by bisection on the CPU oracle) and its two neighbours, and the top of the range, against the
CPU oracle; every sum in [0, 2^24) on the device; 2^24 seeded sums against the device-compiled oracle.

Monotonicity: the oracle's f32 curve itself steps down by one code in a few places with the tonemap on (see
tests/test_oracle_resolve.py); the device must equal it there too, must never drop by more than one code, and must be
monotone with the tonemap off."""
import time

import numpy as np
import pytest

import math_probe as mp
import oracle_binding as ob

pytestmark = pytest.mark.gpu

FLAGS = [0, 2, 4, 6]
SMALL_N = [n for n in mp.RESOLVE_N if n <= 8]
LARGE_N = [n for n in mp.RESOLVE_N if n > 8]


def _check_sweep(n, flags, lo, count):
    bad, viol, first, done, drop = mp.resolve_sweep(n, flags, lo, count)
    assert done == count, (n, flags, done, count)
    assert bad == 0, f"n={n} flags={flags}: {bad} codes differ from the oracle, first at sum {first}"
    assert drop <= 1, f"n={n} flags={flags}: the code drops by {drop}"
    if flags & 2:
        assert viol == 0, f"n={n} flags={flags}: {viol} monotonicity violations without the tonemap"
    return viol


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", SMALL_N)
def test_resolve_every_sum(n, flags):
    t0 = time.perf_counter()
    top = mp.sum_max(n)
    viol = _check_sweep(n, flags, 0, top + 1)
    print(f"\nresolve n={n} flags={flags}: {top + 1} sums, 0 mismatches, {viol} one-code steps down (as the oracle), "
          f"{time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", LARGE_N)
def test_resolve_thresholds_and_seeded_sums(n, flags):
    t0 = time.perf_counter()
    top = mp.sum_max(n)
    t = mp.resolve_thresholds(n, flags)
    edges = np.unique(np.concatenate([t, t - np.uint64(1), t + np.uint64(1),
                                      np.array([top - d for d in range(4096)] + [top - mp.FIXED_MAX * j for j in range(64)],
                                               dtype=np.uint64)]))
    edges = edges[edges <= np.uint64(top)]
    want = ob.resolve_channel(edges, n, flags)
    got = mp.resolve(edges, n, flags, mp.EXACT)
    bad = got != want
    assert not bad.any(), f"n={n} flags={flags}: {int(bad.sum())} differ, first at sum {int(edges[np.argmax(bad)])}"
    _check_sweep(n, flags, 0, 1 << 24)
    rnd = np.random.default_rng(n + flags).integers(0, top, size=1 << 24, dtype=np.uint64, endpoint=True)
    got = mp.resolve(rnd, n, flags, mp.EXACT)
    want = mp.resolve(rnd, n, flags, mp.ORACLE)
    bad = got != want
    assert not bad.any(), f"n={n} flags={flags}: {int(bad.sum())} seeded sums differ, first {int(rnd[np.argmax(bad)])}"
    # the device-compiled oracle is the CPU oracle (a sample of the seeded sums)
    assert (want[:1 << 16] == ob.resolve_channel(rnd[:1 << 16], n, flags)).all()
    print(f"\nresolve n={n} flags={flags}: {int((t <= np.uint64(top)).sum())} thresholds (+-1), {edges.size} edge sums, "
          f"2^24 dense + 2^24 seeded sums, 0 mismatches, {time.perf_counter() - t0:.2f} s")
