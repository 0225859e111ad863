"""mirt-math v1 on the device, function by function: every product function of csrc/mirt_device_math.h (exact build) and
to_fixed is compared ON THE DEVICE with its oracle twin (oracle/mirt_oracle_math.h, compiled for gfx950 by the test-only
probe oracle/mirt_math_probe.hip) over every bit pattern of its domain, and the device-compiled twins are compared with
the CPU oracle on 2^22 stratified inputs per function: product on device == oracle on device == oracle on CPU.
Results are equal when their bits are, or when both are NaN (payloads are not specified)."""
import time

import numpy as np
import pytest

import math_probe as mp
import oracle_binding as ob

pytestmark = pytest.mark.gpu

ALL = (0, 1 << 32)
B = mp.f32_bits
NEG = 0x80000000


def _fixed_operands():
    """24 fixed second operands of atan2: +-0, +-min subnormal, +-FLT_MIN, +-1, +-FLT_MAX, +-inf, NaN, 9 seeded randoms."""
    special = [0.0, -0.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan]
    rnd = np.random.default_rng(11).integers(0, 1 << 32, size=24 - len(special), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([np.array(special, dtype=np.float32), rnd])


def _sin_special():
    """+-0 and the f32 neighbours (+-2 ulp) of k pi / 2 for |k pi / 2| <= 2^20, and the zeros of om_sin_sign among them."""
    k = np.arange(-667544, 667545, dtype=np.float64)
    base = (k * (np.pi / 2)).astype(np.float32).view(np.int32).astype(np.int64)
    cand = np.concatenate([base + d for d in (-2, -1, 0, 1, 2)]).astype(np.uint32).view(np.float32)
    cand = cand[np.abs(cand) <= 2.0 ** 20]
    zeros = cand[ob.sin_sign(cand) == 0]
    rng = np.random.default_rng(5)
    return np.concatenate([np.float32([0.0, -0.0]), zeros, rng.choice(cand, 1 << 16, replace=False)]).astype(np.float32)


def _sweep(name, fn, ranges, params=None):
    t0 = time.perf_counter()
    total = 0
    for lo, count in ranges:
        bad, first, done = mp.sweep(fn, lo, count, params)
        want = count * (len(params) if params is not None and fn not in (mp.SW_POW_PAIRS, mp.SW_SIN_PRODUCT) else 1)
        assert done == want, f"{name}: {done} evaluations, expected {want}"
        assert bad == 0, f"{name}: {bad} mismatches in [{lo:#x}, {lo + count:#x}), first at pattern {first:#010x}"
        total += done
    print(f"\n{name}: {total} evaluations, 0 mismatches, {time.perf_counter() - t0:.2f} s")


SMALL = B(2.0 ** 20) + 1
CASES = {
    "sincos_": (mp.SINCOS, [ALL], None),
    "sincos_small": (mp.SINCOS_SMALL, [(0, SMALL), (NEG, SMALL)], None),
    "sin_sign": (mp.SIN_SIGN, [ALL], None),
    "sin_sign_bits": (mp.SIN_SIGN_BITS, [ALL], None),
    "acos_": (mp.ACOS, [ALL], None),
    "log2_": (mp.LOG2, [ALL], None),
    "exp2_": (mp.EXP2, [ALL], None),
    "exp_": (mp.EXP, [ALL], None),
    "to_fixed": (mp.TO_FIXED, [ALL], None),
    "pow_pos(x, {0.33333, 0.41666666})": (mp.POW_POS, [ALL], np.float32([0.33333, 0.41666666])),
    "rcp_in_range": (mp.RCP_IN_RANGE, [(B(2.0 ** -100), B(2.0 ** 100) - B(2.0 ** -100) + 1),
                                       (NEG | B(2.0 ** -100), B(2.0 ** 100) - B(2.0 ** -100) + 1)], None),
    "sqrt_unit_where(x, true)": (mp.SQRT_UNIT_WHERE, [(1, B(1.0))], None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_exhaustive_against_oracle(name):
    fn, ranges, params = CASES[name]
    _sweep(name, fn, ranges, params)


def test_atan2_every_pattern_against_fixed_operands():
    fixed = _fixed_operands()
    _sweep("atan2_(pattern, x fixed)", mp.SW_ATAN2_Y, [ALL], fixed)
    _sweep("atan2_(y fixed, pattern)", mp.SW_ATAN2_X, [ALL], fixed)


def test_pow_pos_seeded_pairs():
    _sweep("pow_pos seeded pairs", mp.SW_POW_PAIRS, [(0, 1 << 28)], np.float32([3.0]))


def test_pow_unit_on_its_domain():
    ys = np.concatenate([np.float32([0.33333]),
                         np.random.default_rng(3).uniform(0.0, 1.0, 16).astype(np.float32)])
    ys[1:] = np.where(ys[1:] > 0, ys[1:], np.float32(1.0))          # (0, 1]
    lo = B(2.0 ** -32)
    _sweep("pow_unit", mp.POW_UNIT, [(0, 1), (lo, B(1.0) - lo + 1)], ys)


def test_sin_product_negative_seeded_triples():
    _sweep("sin_product_negative", mp.SW_SIN_PRODUCT, [(0, 1 << 28)], _sin_special())


# ---- bridge: the device-compiled oracle twins == the CPU oracle ----

def _stratified(seed: int, per: int = 8192) -> np.ndarray:
    """`per` random mantissas for every exponent and sign (2^22 with per = 8192), plus the edge patterns."""
    rng = np.random.default_rng(seed)
    e = np.repeat(np.arange(512, dtype=np.uint32), per)                 # sign | exponent
    m = rng.integers(0, 1 << 23, size=e.size, dtype=np.uint32)
    x = ((e >> 8) << 31) | ((e & 0xff) << 23) | m
    edges = np.array([0, NEG, 1, NEG | 1, 0x007fffff, 0x00800000, B(1.0), B(-1.0), B(0.5), B(2.0 ** 20), B(-(2.0 ** 20)),
                      B(2.0 ** 20) + 1, B(128.0), B(128.0) - 1, B(-126.0), B(-126.0) + 1, B(-150.0), 0x7f7fffff, 0x7f800000,
                      0xff800000, 0x7fc00000, B(np.pi / 2), B(np.pi), B(2.0 ** -32), B(2.0 ** -100), B(2.0 ** 100)],
                     dtype=np.uint32)
    return np.concatenate([x, edges]).view(np.float32)


def _same(name, got_bits, want, x):
    want_bits = np.ascontiguousarray(want).view(np.uint32)
    g, w = got_bits.view(np.float32), want_bits.view(np.float32)
    bad = (got_bits != want_bits) & ~(np.isnan(g) & np.isnan(w))
    if bad.any():
        i = int(np.argmax(bad))
        pytest.fail(f"{name}: {int(bad.sum())} differ; first input {int(np.float32(x[i]).view(np.uint32)):#010x}: "
                    f"device {int(got_bits[i]):#010x}, CPU {int(want_bits[i]):#010x}")


def test_device_oracle_equals_cpu_oracle():
    x = _stratified(1)
    x2 = np.random.default_rng(2).permutation(x)
    ax, ax2 = np.abs(x), np.abs(x2)
    s, c = ob.sincos(x)
    d0, d1 = mp.eval_fn(mp.SINCOS, mp.ORACLE, x)
    _same("om_sincos (sin)", d0, s, x)
    _same("om_sincos (cos)", d1, c, x)
    _same("om_sin_sign", mp.eval_fn(mp.SIN_SIGN, mp.ORACLE, x)[0], ob.sin_sign(x), x)
    _same("om_acos", mp.eval_fn(mp.ACOS, mp.ORACLE, x)[0], ob.acos(x), x)
    _same("om_atan2", mp.eval_fn(mp.ATAN2, mp.ORACLE, x, x2)[0], ob.atan2(x, x2), x)
    _same("om_log2", mp.eval_fn(mp.LOG2, mp.ORACLE, x)[0], ob.log2(x), x)
    _same("om_exp2", mp.eval_fn(mp.EXP2, mp.ORACLE, x)[0], ob.exp2(x), x)
    _same("om_exp", mp.eval_fn(mp.EXP, mp.ORACLE, x)[0], ob.exp(x), x)
    _same("om_pow_pos", mp.eval_fn(mp.POW_POS, mp.ORACLE, ax, x2)[0], ob.pow_pos(ax, x2), ax)
    _same("to_fixed", mp.eval_fn(mp.TO_FIXED, mp.ORACLE, x)[0], ob.to_fixed(x), x)
    with np.errstate(all="ignore"):
        _same("1 / x", mp.eval_fn(mp.RCP_IN_RANGE, mp.ORACLE, x)[0], np.float32(1.0) / x, x)
        _same("sqrtf", mp.eval_fn(mp.SQRT_UNIT_WHERE, mp.ORACLE, ax)[0], np.sqrt(ax), ax)
    x3 = np.random.default_rng(4).permutation(x)
    want = (ob.sin_sign(x) * ob.sin_sign(x2) * ob.sin_sign(x3) < 0).astype(np.uint32)
    _same("om_sin_sign product", mp.eval_fn(mp.SIN_PRODUCT_NEG, mp.ORACLE, x, x2, x3)[0], want, x)
    # and the product's functions at the same inputs (the sweeps cover them exhaustively; this checks mprobe_eval)
    _same("sincos_ (eval)", mp.eval_fn(mp.SINCOS, mp.EXACT, x)[0], s, x)
    _same("atan2_ (eval)", mp.eval_fn(mp.ATAN2, mp.EXACT, x, x2)[0], ob.atan2(x, x2), x)
    _same("sin_product_negative (eval)", mp.eval_fn(mp.SIN_PRODUCT_NEG, mp.EXACT, x, x2, x3)[0], want, x)
