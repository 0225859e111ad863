"""The OPT-IN fast-math build (MIRT_FLAG_FAST_MATH: hardware v_rcp/v_rsq/v_sqrt/v_sin/v_cos/v_exp/v_log, contraction)
against the default bit-exact build.  No parity claim is made for it; this file measures how far it strays:
per-channel |delta| <= 1 on >= 99.9 % of the pixels of the bench frame at 1000 spp (SURVEY §7's statistical bound),
and it checks that the flag really selects different kernels and stays deterministic."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from helpers import assert_images_equal, scene_data

pytestmark = pytest.mark.gpu


def _histogram(a: np.ndarray, b: np.ndarray) -> dict:
    d = np.abs(a[..., :3].astype(np.int16) - b[..., :3].astype(np.int16)).max(axis=-1)
    vals, counts = np.unique(d, return_counts=True)
    return {int(v): int(c) for v, c in zip(vals, counts)}


@pytest.mark.parametrize("scene,w,h,spp", [("three_spheres", 1920, 1080, 1000), ("earth", 960, 540, 256), ("main_rs_scene", 960, 540, 256),
                                            ("rtiow_final", 480, 270, 64)])
def test_fast_math_stays_within_one_unit(gpu_ctx, scene, w, h, spp):
    sd = scene_data(scene, w, h)
    gpu_ctx.set_scene(sd)
    exact = gpu_ctx.render(m.make_params(w, h, spp, mode=m.MIRT_MODE_PT))
    k_exact = gpu_ctx.last_kernel()
    fast = gpu_ctx.render(m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, flags=m.MIRT_FLAG_FAST_MATH))
    k_fast = gpu_ctx.last_kernel()
    assert k_fast == "fast_build::" + k_exact
    hist = _histogram(exact, fast)
    n = w * h
    within1 = (hist.get(0, 0) + hist.get(1, 0)) / n
    print(f"\nfast-math vs exact, {scene} {w}x{h} {spp} spp: max |delta| per pixel -> pixels {hist}; "
          f"identical {100.0 * hist.get(0, 0) / n:.3f} %, within 1: {100.0 * within1:.4f} %")
    assert within1 >= 0.999, hist
    assert (fast[..., 3] == 255).all()
    # deterministic: integer accumulation and the RNG streams are those of the exact build
    again = gpu_ctx.render(m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, flags=m.MIRT_FLAG_FAST_MATH))
    assert_images_equal(again, fast, "fast-math build is deterministic")


def test_fast_math_is_ignored_where_no_fast_build_exists(gpu_ctx, oracle):
    """Counting launches and parity mode always run the exact build."""
    w, h = 96, 64
    sd = scene_data("three_spheres", w, h)
    gpu_ctx.set_scene(sd)
    p = m.make_params(w, h, 64, mode=m.MIRT_MODE_PT, flags=m.MIRT_FLAG_FAST_MATH | m.MIRT_FLAG_COUNT_WORK)
    img = gpu_ctx.render(p)
    assert not gpu_ctx.last_kernel().startswith("fast_build::")
    assert_images_equal(img, oracle.render(sd, m.make_params(w, h, 64, mode=m.MIRT_MODE_PT)), "counting launch is exact")


# ---- the fast build function by function (the test-only probe, tests/math_probe.py) ----
# Bounds: about twice the worst case measured on the MI355X over these inputs (2^22 seeded per function), against numpy
# float64 of the same f32 inputs:
#   sin, cos on [-4 pi, 4 pi]                              abs   measured 9.17e-7, 8.54e-7
#   acos on [-1, 1]                                        abs   measured 3.11e-7
#   atan2 on [-1, 1]^2                                     abs   measured 2.94e-7
#   log2 on [2^-32, 1]                                     rel   measured 1.19e-7 (relative to max(|log2 x|, 1))
#   exp2 on [-32, 0]                                       rel   measured 8.37e-8
#   pow_unit(x, {0.33333, 0.41666666}), x in [2^-32, 1]    rel   measured 9.31e-7
#   resolve: fast and exact codes differ by at most one at every threshold +-1 and at 2^20 seeded sums (measured: one
#   with the tonemap or the sRGB curve on, none with both off).
FAST_BOUNDS = {"sin": 2e-6, "cos": 2e-6, "acos": 6.5e-7, "atan2": 6e-7, "log2": 2.4e-7, "exp2": 1.7e-7, "pow": 1.9e-6}


def _fast_errors():
    import math_probe as mp
    rng = np.random.default_rng(17)
    n = 1 << 22
    out = {}
    x = rng.uniform(-4 * np.pi, 4 * np.pi, n).astype(np.float32)
    s, c = mp.eval_f32(mp.SINCOS, mp.FAST, x)
    out["sin"] = np.abs(s - np.sin(x.astype(np.float64))).max()
    out["cos"] = np.abs(c - np.cos(x.astype(np.float64))).max()
    x = rng.uniform(-1, 1, n).astype(np.float32)
    out["acos"] = np.abs(mp.eval_f32(mp.ACOS, mp.FAST, x)[0] - np.arccos(x.astype(np.float64))).max()
    y = rng.uniform(-1, 1, n).astype(np.float32)
    out["atan2"] = np.abs(mp.eval_f32(mp.ATAN2, mp.FAST, y, x)[0] - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max()
    x = np.exp2(rng.uniform(-32, 0, n)).astype(np.float32)
    ref = np.log2(x.astype(np.float64))
    out["log2"] = (np.abs(mp.eval_f32(mp.LOG2, mp.FAST, x)[0] - ref) / np.maximum(np.abs(ref), 1.0)).max()
    y = rng.uniform(-32, 0, n).astype(np.float32)
    ref = np.exp2(y.astype(np.float64))
    out["exp2"] = (np.abs(mp.eval_f32(mp.EXP2, mp.FAST, y)[0] - ref) / ref).max()
    e = np.where(rng.random(n) < 0.5, np.float32(0.33333), np.float32(0.41666666)).astype(np.float32)
    ref = np.power(x.astype(np.float64), e.astype(np.float64))
    out["pow"] = (np.abs(mp.eval_f32(mp.POW_UNIT, mp.FAST, x, e)[0] - ref) / ref).max()
    return {k: float(v) for k, v in out.items()}


def test_fast_math_functions_within_bounds():
    err = _fast_errors()
    print("\nfast build, largest error per function: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= FAST_BOUNDS[k], (k, v, FAST_BOUNDS[k])


@pytest.mark.parametrize("flags", [0, 2, 4, 6])
def test_fast_resolve_within_one_code(flags):
    import math_probe as mp
    worst = 0
    for n in mp.RESOLVE_N:
        t = mp.resolve_thresholds(n, flags)
        rnd = np.random.default_rng(n ^ flags).integers(0, mp.sum_max(n), size=1 << 20, dtype=np.uint64, endpoint=True)
        s = np.concatenate([t, t - np.uint64(1), t + np.uint64(1), rnd])
        s = s[s <= np.uint64(mp.sum_max(n))]
        d = np.abs(mp.resolve(s, n, flags, mp.FAST).astype(np.int16) - mp.resolve(s, n, flags, mp.EXACT).astype(np.int16))
        worst = max(worst, int(d.max()))
        assert d.max() <= 1, (n, flags, int(s[np.argmax(d)]))
    print(f"\nfast resolve flags={flags}: largest |fast - exact| {worst} code")
