"""Worlds for the mirt_ctx_set_spheres tests whose always-tested list sits on an edge of the host rule (csrc/mirt_bvh.cpp:
bvh_always_list; tests/bvh_check.py: always_list).  Host-side data only.  ALWAYS_WORLDS: name -> (builder, the length of the list the
world is made to have); tests/test_set_spheres_abi.py holds every world to its claim with the host rule alone."""
from __future__ import annotations

import numpy as np

from hbm_worlds import sphere_array

N_MATS = 7                 # hbm_worlds.field_materials


def _f32_below(limit: float) -> np.float32:
    """The largest float32 whose value is < limit."""
    f = np.float32(limit)
    return f if float(f) < limit else np.nextafter(f, np.float32(0))


EDGE_BELOW = _f32_below(3.0e38)                                 # |c| + r stays below 3.0e38 in fp64 for a small r: a finite box
EDGE_AT = np.nextafter(EDGE_BELOW, np.float32(np.inf))          # the first float32 >= 3.0e38: not finite by the rule
assert float(EDGE_BELOW) + 0.25 < 3.0e38 <= float(EDGE_AT) + 0.25


def _base(n, seed, radius=(0.1, 0.3)):
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-4, 4, (n, 3))
    cen[:, 2] -= 6
    return rng, cen.astype(np.float32), rng.uniform(*radius, n).astype(np.float32), rng.integers(0, N_MATS, n)


def non_finite(k: int, n: int = 300, seed: int = 31):
    """k spheres without a finite box scattered through n -- a NaN radius, an infinite radius, an infinite or NaN centre component, a
    centre at the first float at or above 3.0e38 (either sign) -- and, in front of each of the first three, a sphere whose centre is
    the last float BELOW 3.0e38: finite by the rule, so a key that called it bad would move the list."""
    rng, cen, rad, mat = _base(n, seed)
    bad = np.sort(rng.choice(np.arange(8, n), k, replace=False))
    for j, i in enumerate(bad):
        kind = j % 6
        if kind == 0: rad[i] = np.nan
        elif kind == 1: cen[i, j % 3] = np.inf
        elif kind == 2: cen[i, (j + 1) % 3] = EDGE_AT
        elif kind == 3: rad[i] = -np.inf
        elif kind == 4: cen[i, (j + 2) % 3] = -EDGE_AT
        else: cen[i, j % 3] = np.nan
    free = np.setdiff1d(np.arange(n), bad)
    for j, i in enumerate(free[:3]):                                # indices below every bad one
        cen[i, j] = EDGE_BELOW if j != 1 else -EDGE_BELOW
        rad[i] = 0.25
    return sphere_array(cen, rad, mat)


def shared_cap(seed: int = 32):
    """60 non-finite and 10 big spheres, 6 of them of one radius: 4 big are taken -- the two larger ones, then the tied ones at the two
    lowest indices (placed out of order among the others)."""
    n = 300
    rng, cen, rad, mat = _base(n, seed)
    idx = rng.permutation(n)
    rad[idx[:60]] = np.nan
    big = idx[60:70]
    rad[big[0]], rad[big[1]] = 9.0, -8.0
    rad[big[2:8]] = 5.0
    rad[big[8]], rad[big[9]] = 4.5, 4.0
    return sphere_array(cen, rad, mat)


def shared_cap_expected():
    a = shared_cap()
    rng, *_ = _base(300, 32)
    idx = rng.permutation(300)
    big = idx[60:70]
    return a, np.sort(np.concatenate([idx[:60], big[:2], np.sort(big[2:8])[:2]]))


def equal_radii():
    _, cen, rad, mat = _base(200, 33)
    rad[:] = 0.25
    return sphere_array(cen, rad, mat)


def four_medians():
    """median 0.25: a radius of exactly 1.0 is not above 4 medians, the next float is."""
    _, cen, rad, mat = _base(101, 34)
    rad[:] = 0.25
    rad[40] = 1.0
    rad[70] = np.nextafter(np.float32(1.0), np.float32(2.0))
    rad[20] = -1.0
    return sphere_array(cen, rad, mat)


def upper_median():
    """10 finite spheres, middle radii 0.3 (position 4) and 0.5 (position 5): the rule takes position 5, so the limit is 2.0 and only
    2.5 is above it; the lower median would take 1.5 too."""
    _, cen, rad, mat = _base(10, 35)
    rad[:] = np.asarray([0.5, 0.25, 2.5, 0.25, 0.5, 1.5, 0.3, 0.25, 0.5, 0.25], np.float32)
    return sphere_array(cen, rad, mat)


def signed_radii():
    """|r| decides: 14 of +-0.25, two each of 0.0 and -0.0, and -3.0, 2.0 (taken), -1.0 (exactly 4 medians: not taken)."""
    _, cen, rad, mat = _base(21, 36)
    rad[:] = np.asarray([0.25, -0.25] * 7 + [0.0, -0.0, 0.0, -0.0, -3.0, 2.0, -1.0], np.float32)[np.random.default_rng(36).permutation(21)]
    return sphere_array(cen, rad, mat)


def zero_median():
    """10 of 15 radii are 0.0 or -0.0: the median is 0, and every radius above it is big."""
    _, cen, rad, mat = _base(15, 37)
    rad[:] = np.asarray([0.0, -0.0] * 5 + [0.2, -0.3, 0.4, 1e-30, -0.25], np.float32)[np.random.default_rng(37).permutation(15)]
    return sphere_array(cen, rad, mat)


def eighty_big():
    """80 spheres above 4 medians, all different: the 64 largest are taken."""
    rng, cen, rad, mat = _base(300, 38)
    rad[:] = 0.1
    big = rng.choice(300, 80, replace=False)
    rad[big] = (1.0 + 0.01 * rng.permutation(80)).astype(np.float32) * np.where(np.arange(80) % 3 == 0, -1, 1)
    return sphere_array(cen, rad, mat)


ALWAYS_WORLDS = {
    "64 non-finite": (lambda: non_finite(64), 64),
    "65 non-finite": (lambda: non_finite(65), 64),
    "70 non-finite": (lambda: non_finite(70), 64),
    "10 non-finite": (lambda: non_finite(10), 10),                # room left, and nothing above 4 medians
    "60 non-finite + 10 big, 6 tied": (shared_cap, 64),
    "equal radii": (equal_radii, 0),
    "exactly 4 medians": (four_medians, 1),
    "upper median": (upper_median, 1),
    "negative and zero radii": (signed_radii, 2),
    "median 0": (zero_median, 5),
    "80 big": (eighty_big, 64),
}
