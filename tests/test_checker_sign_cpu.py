"""The guarded fast path of sin_product_negative (csrc/mirt_device_math.h: sin_product_decided), axis by axis, restated in numpy
and held to the oracle's sin_sign: wherever the fast path calls an input decided, the parity of floor(a * fl(1/pi)) is the sign
the full reduction gives, and that sign is not zero.  Agreement per axis implies agreement of the product of three; the
undecided lanes run the reduction itself.  The device runs the same comparison over all 2^32 patterns
(tests/test_gpu_checker_sign.py); here the inputs are the ones where it can go wrong -- the neighbours of every multiple of
pi in the reduction's domain and the edges of that domain -- plus a seeded sample, and two coverage conditions keep the test
from passing because nothing is decided."""
import re
from pathlib import Path

import numpy as np

import oracle_binding as ob

ROOT = Path(__file__).resolve().parent.parent
DEVICE_H = (ROOT / "weekend-raytracer-wgpu_amd" / "csrc" / "mirt_device_math.h").read_text()

F = np.float32
FRAC_1_PI = F(0.31830987)
ONE_BELOW = F(1.0) - F(2.0 ** -24)          # v_fract_f32 never returns 1.0


def _constant(pattern: str) -> float:
    m = re.search(pattern, DEVICE_H)
    assert m, pattern
    return float.fromhex(m.group(1)) if "0x" in m.group(1) else float(m.group(1))


BAND = F(_constant(r"#define MIRT_CHECKER_BAND\s+(0x[0-9a-fp.+-]+)f"))
MAX_T = F(_constant(r"kCheckerMaxT\s*=\s*([0-9.]+)f"))


def fast_axis(a, band=None):
    """(decided, odd) of one axis, operation by operation as the device computes them in binary32."""
    band = BAND if band is None else F(band)
    a = np.ascontiguousarray(a, dtype=F)
    with np.errstate(all="ignore"):
        t = a * FRAC_1_PI
        n = np.floor(t)
        fr = np.minimum(t - n, ONE_BELOW)            # NaN for NaN and inf
        thr = band * np.abs(t)
        decided = (fr > thr) & ((F(1.0) - fr) > thr) & (np.abs(t) <= MAX_T)
        odd = np.where(decided, np.mod(n, F(2.0)) != 0, False)
    return decided, odd


def _disagreements(a):
    decided, odd = fast_axis(a)
    s = ob.sin_sign(a)
    return a[decided & ((s == 0) | ((s < 0) != odd))], int(decided.sum())


def _pi_neighbours(ulps: int = 64) -> np.ndarray:
    """Every f32 within `ulps` of k pi for |k pi| <= 2^20 (and a little beyond), as tests/test_gpu_math_exhaustive.py lists k pi/2."""
    k = np.arange(-333780, 333781, dtype=np.float64)
    base = (k * np.pi).astype(F).view(np.int32).astype(np.int64)
    return np.concatenate([(base + d).astype(np.uint32).view(F) for d in range(-ulps, ulps + 1)])


def _edges() -> np.ndarray:
    sub = np.array([1, 2, 0x7fffff, 0x800000, 0x800001], dtype=np.uint32)
    top = np.float32(2.0 ** 20).view(np.uint32) + np.arange(-64, 65, dtype=np.int64).astype(np.uint32)
    pos = np.concatenate([sub, top]).view(F)
    big = F([2.0 ** 21, 1.0e7, 3.0e38, np.inf, np.nan, 0.0])
    x = np.concatenate([pos, big])
    return np.concatenate([x, -x])


def test_constants_are_the_headers():
    assert BAND == F(2.0 ** -21) and MAX_T == F(333772.0)
    assert f"{float(FRAC_1_PI)!r}"[:10] in DEVICE_H          # kFrac1Pi = 0.31830987f
    # |t| <= MAX_T keeps |a| inside the reduction's domain, with the rounding of t against it
    assert float(MAX_T) / (float(FRAC_1_PI) * (1.0 - 2.0 ** -24)) < 2.0 ** 20


def test_decided_inputs_agree_next_to_every_multiple_of_pi():
    a = np.concatenate([_pi_neighbours(), _edges()])
    bad, decided = _disagreements(a)
    print(f"\n{a.size} inputs, {decided} decided")
    assert bad.size == 0, f"{bad.size} decided inputs disagree, first {bad[:4]!r}"
    # none of the inputs the reduction calls zero, clamps or cannot order is decided
    d, _ = fast_axis(_edges())
    e = _edges()
    assert not d[~(np.abs(e) <= F(2.0 ** 20)) | (e == 0)].any()


def test_decided_inputs_agree_on_a_seeded_sample():
    rng = np.random.default_rng(2024)
    n = 10_000_000
    mag = np.exp2(rng.uniform(-30.0, 21.0, n))
    a = (mag * rng.choice([-1.0, 1.0], n)).astype(F)
    bad, decided = _disagreements(a)
    print(f"\n{n} inputs, {decided} decided")
    assert bad.size == 0, f"{bad.size} decided inputs disagree, first {bad[:4]!r}"


def test_the_band_leaves_nearly_everything_decided():
    for span, share in ((64.0, 0.999), (4096.0, 0.99)):
        a = np.linspace(-span, span, 4_000_001).astype(F)
        decided, _ = fast_axis(a)
        got = decided.mean()
        print(f"\n[-{span:g}, {span:g}]: {got:.6f} decided")
        assert got >= share
