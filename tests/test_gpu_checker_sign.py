"""The checkerboard's guarded fast sign path on the device (csrc/mirt_device_math.h: sin_product_negative).

1. mirt_ctx_selftest_checker_sign: over ALL 2^32 binary32 patterns, as one axis, no input the fast path calls decided has a
   parity that disagrees with the sign of the full reduction, none is a zero of the reduction, and the decided inputs are
   more than 99 % of the finite inputs inside the reduction's domain (|a| <= 2^20) -- the check is not vacuous.
2. Exact 64-bit sums against the oracle on checker grounds where the sign is decided near the camera, at the horizon
   (|t| in the hundreds), at coordinates scaled by 2^10 and 2^-10, and beyond the 2^20 clamp (sin = 0 by the spec), through
   every schedule: default, strip, streaming, pool, and the grid build with a 40-sphere soup on the ground."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from helpers import _flattened, simple_camera

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 8
COUNTERS = ["rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses"]
CHECKER, METAL, GLASS = 0, 2, 3                # main_rs_materials(): the checker is the ground's material


def test_every_decided_input_has_the_reductions_sign(gpu_ctx):
    decided, mismatches, zeros = gpu_ctx.selftest_checker_sign()
    finite_in_domain = 2 * (int(np.float32(2.0 ** 20).view(np.uint32)) + 1)          # +-0 .. +-2^20
    print(f"\ndecided {decided} of {finite_in_domain} in the domain ({decided / finite_in_domain:.6f}), "
          f"mismatches {mismatches}, zeros {zeros}")
    assert mismatches == 0 and zeros == 0
    assert decided <= finite_in_domain
    assert decided > 0.99 * finite_in_domain


def _world(ground_c, ground_r, eye, direction, scale=1.0, shift=(0.0, 0.0, 0.0), soup=False, focus=10.0):
    """Config 3's three spheres with the given ground, optionally 40 small spheres resting on it, moved by `shift` and then
    multiplied by `scale` together with the camera; eye = None: the default fly camera (unmoved worlds only)."""
    _, cam, mats, tex = _flattened("three_spheres")
    shift = np.asarray(shift, np.float64)
    world = [(ground_c, ground_r, CHECKER), ((0.0, 1.0, 0.0), 1.0, GLASS), ((-5.0, 1.0, 0.0), 1.0, METAL)]
    if soup:
        rng = np.random.default_rng(40)
        for _ in range(40):
            r = float(rng.uniform(0.1, 0.3))
            x, z = rng.uniform(-6.0, 6.0, 2)
            gc = np.asarray(ground_c, np.float64)
            y = gc[1] + np.sqrt(max(ground_r ** 2 - (x - gc[0]) ** 2 - (z - gc[2]) ** 2, 0.0)) + r       # resting on the ground
            world.append(((x, y, z), r, int(rng.choice([CHECKER, METAL, GLASS]))))
    spheres = [m.Sphere.new(tuple((np.asarray(c, np.float64) + shift) * scale), float(r * scale), k).to_c() for c, r, k in world]
    if eye is None:
        camera = m.GpuCamera.new(cam, (W, H)).c
    else:
        camera = simple_camera(W, H, eye=tuple((np.asarray(eye, np.float64) + shift) * scale), direction=direction, vfov=50.0,
                               aperture=0.0, focus=focus * scale)
    return m.SceneData(camera, spheres, list(mats), tex)


GROUND3 = ((0.0, -500.0, -1.0), 500.0)
NEAR = dict(eye=(0.0, 2.0, 9.0), direction=(0.0, -0.15, -1.0))
GROUNDS = {
    "config 3": lambda soup: _world(*GROUND3, eye=None, direction=None, soup=soup),
    "horizon": lambda soup: _world(*GROUND3, eye=(0.0, 30.0, 120.0), direction=(0.0, -0.12, -1.0), soup=soup, focus=120.0),
    "scaled 2^10": lambda soup: _world(*GROUND3, scale=2.0 ** 10, soup=soup, **NEAR),
    "scaled 2^-10": lambda soup: _world(*GROUND3, scale=2.0 ** -10, soup=soup, **NEAR),
    "radius 1e6": lambda soup: _world((0.0, -1.0e6, -1.0), 1.0e6, soup=soup, **NEAR),
    # the same ground where 5 x exceeds 2^20: the spec's sine is 0 there and the lanes are never decided
    "radius 1e6 past the clamp": lambda soup: _world((0.0, -1.0e6, -1.0), 1.0e6, shift=(2.5e5, 0.0, 0.0), soup=soup, **NEAR),
}


@pytest.fixture(scope="module")
def stream_ctx():
    import os
    old = os.environ.get("MIRT_STREAM")
    os.environ["MIRT_STREAM"] = "1"             # tuning knobs are read once, in mirt_ctx_create
    try:
        ctx = m.Context(0)
    finally:
        if old is None:
            os.environ.pop("MIRT_STREAM", None)
        else:
            os.environ["MIRT_STREAM"] = old
    yield ctx
    ctx.close()


def _sums(ctx, p):
    ctx.accum_reset(p)
    ctx.accum_add(p)
    return ctx.accum_read(p)


@pytest.mark.parametrize("soup", [False, True], ids=["flat", "grid soup"])
@pytest.mark.parametrize("ground", list(GROUNDS))
def test_exact_sums_on_checker_grounds(gpu_ctx, stream_ctx, oracle, ground, soup):
    sd = GROUNDS[ground](soup)
    gpu_ctx.set_scene(sd)
    stream_ctx.set_scene(sd)
    kernels = set()
    for spp in (32, 64):
        want = oracle.render_pt_sums(sd, m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=BOUNCES))
        for name, ctx, flags in (("default", gpu_ctx, 0), ("strip", gpu_ctx, m.MIRT_FLAG_KERNEL_STRIP),
                                 ("pool", gpu_ctx, m.MIRT_FLAG_KERNEL_POOL), ("stream", stream_ctx, 0)):
            p = m.make_params(W, H, spp, mode=m.MIRT_MODE_PT, num_bounces=BOUNCES, flags=flags)
            got = _sums(ctx, p)
            kernels.add(ctx.last_kernel())
            assert np.array_equal(got, want), f"{ground}, {name}, {spp} spp: {int((got != want).any(-1).sum())} pixels differ ({ctx.last_kernel()})"
    print(f"\n{ground}, soup {soup}: {sorted(kernels)}")
    assert any("strip" in k for k in kernels) and any("pool" in k for k in kernels)
    assert soup or any("stream" in k for k in kernels)            # the streaming build serves flat scenes only
    # the counting builds: every branch decision of every path, against the oracle's counters
    p = m.make_params(W, H, 32, mode=m.MIRT_MODE_PT, num_bounces=BOUNCES, flags=m.MIRT_FLAG_COUNT_WORK)
    want_img = oracle.render(sd, p)
    want_counts = oracle.stats()
    for flags in (m.MIRT_FLAG_KERNEL_STRIP, m.MIRT_FLAG_KERNEL_POOL):
        pc = m.make_params(W, H, 32, mode=m.MIRT_MODE_PT, num_bounces=BOUNCES, flags=flags | m.MIRT_FLAG_COUNT_WORK)
        assert np.array_equal(gpu_ctx.render(pc), want_img), f"{ground}: counting build, flags {flags:#x}"
        st = gpu_ctx.stats()
        assert {k: st[k] for k in COUNTERS} == {k: want_counts[k] for k in COUNTERS}, f"{ground}: counters, flags {flags:#x}"
    assert want_counts["scatter"][3] > 1000          # the checkerboard routine ran
