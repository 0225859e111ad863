"""The oracle's resolve curve (oracle/mirt_oracle_resolve.h: mean -> uncharted2 -> sRGB OETF -> round to nearest) against
a float64 evaluation of the same curve, on the bisection grid of its 255 thresholds (tests/math_probe.py).

Measured on this grid (every threshold +-1, [0, 2^16) and 2^16 seeded sums; all sample counts and flags): the f32 codes
differ from floor(255 v + 0.5) in float64 by at most one code, and only where the float64 value of 255 v + 0.5 lies
within 7.93e-5 of an integer (the largest distance, with the tonemap; 1.8e-5 without it).  The bound below is 2.5x that.

The f32 curve is NOT monotone everywhere: uncharted2's quotient minus a constant (num / den - 0.02 / 0.30, wgsl:94-103)
cancels, and its f32 rounding can step the code down by one where the float64 value is within that distance of a
boundary (a few dozen places per sample count).  The shader evaluates the same f32 expression.  Without the tonemap the
curve is monotone on the grid."""
import numpy as np
import pytest

import math_probe as mp
import oracle_binding as ob

DELTA = 2.0e-4
FLAGS = [0, 2, 4, 6]      # MIRT_FLAG_NO_TONEMAP = 2, MIRT_FLAG_NO_SRGB = 4


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", mp.RESOLVE_N)
def test_oracle_resolve_against_float64(n, flags):
    g = mp.resolve_grid(n, flags, seed=1, n_random=1 << 16, dense=1 << 16)
    code = ob.resolve_channel(g, n, flags).astype(np.int64)
    x = mp.resolve_f64(g, n, flags)
    c64 = np.minimum(np.floor(x), 255).astype(np.int64)
    d = code - c64
    assert np.abs(d).max() <= 1, (n, flags, int(g[np.argmax(np.abs(d))]))
    off = d != 0
    dist = np.abs(x - np.round(x))
    assert (dist[off] < DELTA).all(), \
        f"n={n} flags={flags}: code differs from float64 at sum {int(g[off][np.argmax(dist[off])])}, {dist[off].max():.3e} from a boundary"
    # the top of the range saturates, 0 is black
    assert code[0] == 0 and ob.resolve_channel(np.uint64([mp.sum_max(n)]), n, flags)[0] == 255


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("n", mp.RESOLVE_N)
def test_oracle_resolve_is_monotone_up_to_one_code(n, flags):
    g = mp.resolve_grid(n, flags, seed=2, n_random=1 << 16, dense=1 << 16)
    code = ob.resolve_channel(g, n, flags).astype(np.int64)
    step = np.diff(code)
    assert step.min() >= -1, (n, flags, int(g[np.argmin(step)]))
    if flags & 2:                                   # no tonemap: monotone
        assert step.min() >= 0, (n, flags, int(g[np.argmin(step)]))
    # every decrease sits within DELTA of a float64 boundary
    x = mp.resolve_f64(g, n, flags)
    i = np.nonzero(step < 0)[0]
    near = np.minimum(np.abs(x[i] - np.round(x[i])), np.abs(x[i + 1] - np.round(x[i + 1])))
    assert (near < DELTA).all(), (n, flags)
    # the bisection found every code the curve reaches, in order
    t = mp.resolve_thresholds(n, flags)
    assert (np.diff(t.astype(np.float64)) >= 0).all()
    reached = t <= np.uint64(mp.sum_max(n))
    assert reached.all(), (n, flags, int((~reached).sum()))
    assert (ob.resolve_channel(t, n, flags).astype(np.int64) >= np.arange(1, 256)).all()


def test_oracle_to_fixed_edges():
    x = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1.0, 4095.9998, 4096.0, 1e30, 2.0 ** -20, 2.0 ** -21, 0.5],
                 dtype=np.float32)
    want = [0, 0, 0, 0, mp.FIXED_MAX, 0, 1 << 20, int(np.float32(4095.9998) * np.float32(1048576.0)), mp.FIXED_MAX, mp.FIXED_MAX,
            1, 0, 1 << 19]
    assert ob.to_fixed(x).tolist() == want


def test_oracle_sin_sign_and_exp_bindings():
    x = np.array([0.0, -0.0, 1.0, -1.0, 3.0, 4.0, 1e30, np.nan], dtype=np.float32)
    assert ob.sin_sign(x).tolist() == [0, 0, 1, -1, 1, -1, 0, 0]
    s, _ = ob.sincos(x[:6])
    assert (np.sign(s[2:]) == ob.sin_sign(x[2:6])).all()
    e = ob.exp(np.float32([0.0, 1.0, -1.0, 10.0]))
    assert e[0] == 1.0 and np.allclose(e, np.exp([0.0, 1.0, -1.0, 10.0]), rtol=3e-7)
    assert (ob.exp(np.float32([0.5])) == ob.exp2(np.float32([0.5]) * np.float32(1.44269504))).all()
