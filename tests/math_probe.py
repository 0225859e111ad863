"""ctypes binding of the test-only device probe (oracle/_build/libmirt_math_probe.so, oracle/mirt_math_probe.hip).  TEST
INFRASTRUCTURE: the product's elementary functions (exact and fast build) and its resolve, and the oracle's sequences
compiled for the device, evaluated on given inputs or compared on the device over whole ranges of bit patterns."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PATH = ROOT / "oracle" / "_build" / "libmirt_math_probe.so"

# function ids (enum MprobeFn / MprobeSweepFn of mirt_math_probe.hip)
SINCOS, SINCOS_SMALL, SIN_SIGN, SIN_SIGN_BITS, SIN_PRODUCT_NEG = 0, 1, 2, 3, 4
ACOS, ATAN2, LOG2, EXP2, EXP, POW_POS, POW_UNIT, RCP_IN_RANGE, SQRT_UNIT_WHERE, TO_FIXED = 5, 6, 7, 8, 9, 10, 11, 12, 13, 14
SW_ATAN2_Y, SW_ATAN2_X, SW_POW_PAIRS, SW_SIN_PRODUCT = 100, 101, 102, 103
EXACT, FAST, ORACLE = 0, 1, 2
NONE = (1 << 64) - 1                      # "no mismatch" of the smallest-mismatch fields

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not PATH.exists():
            subprocess.run(["make", "-C", str(ROOT / "oracle")], check=True, capture_output=True)
        L = C.CDLL(str(PATH))
        P = C.POINTER
        fp, u32p, u64p = P(C.c_float), P(C.c_uint32), P(C.c_ulonglong)
        L.mprobe_eval.restype = C.c_int
        L.mprobe_eval.argtypes = [C.c_int, C.c_int, fp, fp, fp, u32p, u32p, C.c_uint64]
        L.mprobe_sweep.restype = C.c_int
        L.mprobe_sweep.argtypes = [C.c_int, C.c_uint64, C.c_uint64, fp, C.c_uint32, u64p]
        L.mprobe_resolve.restype = C.c_int
        L.mprobe_resolve.argtypes = [P(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, P(C.c_uint8)]
        L.mprobe_resolve_sweep.restype = C.c_int
        L.mprobe_resolve_sweep.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u64p]
        _lib = L
    return _lib


def _check(err: int, what: str) -> None:
    if err != 0:
        raise RuntimeError(f"{what}: hipError_t {err}")


def _f32(a):
    if a is None:
        return None
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def eval_fn(fn: int, build: int, a, b=None, c=None):
    """(out0, out1) as uint32 bit patterns: the function of `build` (EXACT, FAST or the device-compiled ORACLE twin)."""
    a, b, c = _f32(a), _f32(b), _f32(c)
    n = a.size
    o0, o1 = np.empty(n, np.uint32), np.empty(n, np.uint32)
    up = lambda o: o.ctypes.data_as(C.POINTER(C.c_uint32))       # noqa: E731
    _check(lib().mprobe_eval(fn, build, _fp(a), _fp(b), _fp(c), up(o0), up(o1), n), f"mprobe_eval({fn}, {build})")
    return o0, o1


def eval_f32(fn: int, build: int, a, b=None, c=None):
    o0, o1 = eval_fn(fn, build, a, b, c)
    return o0.view(np.float32), o1.view(np.float32)


def sweep(fn: int, lo: int, count: int, params=None) -> tuple[int, int, int]:
    """(mismatches, smallest mismatching pattern or NONE, evaluations): the exact build vs its oracle twin on the device."""
    p = _f32(params)
    out = (C.c_ulonglong * 3)()
    _check(lib().mprobe_sweep(fn, lo, count, _fp(p), 0 if p is None else p.size, out), f"mprobe_sweep({fn})")
    return int(out[0]), int(out[1]), int(out[2])


def resolve(sums, n_samples: int, flags: int, build: int) -> np.ndarray:
    s = np.ascontiguousarray(sums, dtype=np.uint64)
    out = np.empty(s.size, np.uint8)
    _check(lib().mprobe_resolve(s.ctypes.data_as(C.POINTER(C.c_uint64)), s.size, n_samples, flags, build,
                                out.ctypes.data_as(C.POINTER(C.c_uint8))), "mprobe_resolve")
    return out


def resolve_sweep(n_samples: int, flags: int, lo: int, count: int) -> tuple[int, int, int, int, int]:
    """(mismatches, monotonicity violations, smallest mismatching sum or NONE, sums evaluated, largest drop of a code)."""
    out = (C.c_ulonglong * 5)()
    _check(lib().mprobe_resolve_sweep(n_samples, flags, lo, count, out), "mprobe_resolve_sweep")
    return tuple(int(v) for v in out)


def f32_bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


# ---- the resolve curve's grid (CPU oracle; shared by tests/test_oracle_resolve.py and tests/test_gpu_resolve.py) ----
RESOLVE_N = [1, 2, 3, 7, 63, 64, 65, 1000, 4000, 1 << 20, 1 << 31, (1 << 31) + 1, (1 << 32) - 1]
FIXED_MAX = 4294967040                     # the largest per-sample value of to_fixed (the largest f32 below 2^32)


def sum_max(n: int) -> int:
    return n * FIXED_MAX


def resolve_thresholds(n: int, flags: int) -> np.ndarray:
    """t[k - 1] = the smallest sum whose oracle code is >= k, k = 1..255, by bisection over [0, n * FIXED_MAX];
    sum_max(n) + 1 where no sum reaches k.  Meaningful only for a monotone curve (test_oracle_resolve checks it)."""
    import oracle_binding as ob
    k = np.arange(1, 256)
    lo = np.zeros(255, np.uint64)
    hi = np.full(255, sum_max(n) + 1, np.uint64)
    while (lo < hi).any():
        mid = lo + (hi - lo) // np.uint64(2)
        ge = ob.resolve_channel(mid, n, flags).astype(np.int64) >= k
        act = lo < hi
        hi = np.where(act & ge, mid, hi)
        lo = np.where(act & ~ge, mid + np.uint64(1), lo)
    return lo


def resolve_grid(n: int, flags: int, seed: int = 0, n_random: int = 1 << 24, dense: int = 1 << 24) -> np.ndarray:
    """Sorted unique sums: every threshold and its two neighbours, every sum in [0, dense), `n_random` seeded sums,
    and the top of the range (the largest sums to_fixed can produce)."""
    top = sum_max(n)
    t = resolve_thresholds(n, flags)
    parts = [t, t - np.uint64(1), t + np.uint64(1), np.arange(0, min(dense, top + 1), dtype=np.uint64)]
    rng = np.random.default_rng(seed + 7919 * n + flags)
    parts.append(rng.integers(0, top, size=n_random, dtype=np.uint64, endpoint=True))
    parts.append(np.array([max(top - d, 0) for d in range(4096)] + [top - FIXED_MAX * j for j in range(min(n, 64))],
                          dtype=np.uint64))
    g = np.unique(np.concatenate(parts))
    return g[g <= np.uint64(top)]


def resolve_f64(sums, n: int, flags: int) -> np.ndarray:
    """255 * v + 0.5 in float64, v = the resolve curve as the shader writes it (mean -> uncharted2 -> sRGB OETF, clamped to
    [0, 1]); its floor is the float64 code."""
    m = np.asarray(sums, dtype=np.float64) / (float(n) * 1048576.0)

    def tonemap(x):
        return (x * (0.15 * x + 0.05) + 0.004) / (x * (0.15 * x + 0.50) + 0.06) - 0.02 / 0.30

    if not flags & 2:                      # MIRT_FLAG_NO_TONEMAP
        m = tonemap(0.246 * m) / tonemap(11.2)
    if not flags & 4:                      # MIRT_FLAG_NO_SRGB
        with np.errstate(invalid="ignore"):
            m = np.where(m > 0.0031308, 1.055 * np.power(np.maximum(m, 0.0), 1.0 / 2.4) - 0.055, 12.92 * m)
    return 255.0 * np.clip(m, 0.0, 1.0) + 0.5
