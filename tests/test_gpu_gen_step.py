"""The pooled kernel's GEN step (MI355X).  A strip's prologue writes one record per pixel -- (float)x, (float)y and the pixel's part of
the seed, (x + y * width) ^ seed_mix -- into spare words of the wave's path slots, and every GEN step reads its pixel's record instead
of deriving the three from the strip's addressing again; the seed stays jenkins_hash(pixel part ^ jenkins_hash(sample + 1)).  That
changes no number, so every case compares the exact 64-bit sums or the u8 image with the oracle -- at the smallest shapes where it can
go wrong: a non-zero seed, strips that wrap rows, the addressing of frames narrower than a strip, a ragged last strip, the narrow
end-of-frame strips, bands and tile partitions, first samples from 0 to the last index the ABI admits, one small case per build of the
kernel text (the grid build keeps no records: its slots use those words), and two contexts on one device.  MIRT_FLAG_KERNEL_POOL makes
small frames run the pooled kernel.

The first-sample cases sit around 65 536, where a table of hashed sample indices -- measured beside the records and not built, DESIGN.md
4.5 -- would have ended.  The progressive calls (mirt_ctx_accum_*) continue at the context's own sample count, so cases with a
`sample_begin` compare images.  A launch with sample_begin = 0xFFFFFFF0 and spp = 40 -- where sample + 1 would wrap -- is refused by the
library and by the oracle alike (sample_begin + spp may not pass 2^32 - 1): that is asserted, and the launch that ends at the last index
there is, 0xFFFFFFFE, is compared."""
from functools import lru_cache

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from grid_rounding import _scene as soup_scene, sphere_soup
from hbm_worlds import look
from helpers import assert_images_equal, scene_data

pytestmark = pytest.mark.gpu

POOL = m.MIRT_FLAG_KERNEL_POOL
ENTRIES = 65536                              # see above
W, H, SPP = 48, 20, 40
DEFAULT_BUILD = "render_pt_pool_kernel<256,112,6,false,false,3,false,false>"
COUNTERS = ["rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses"]


def _pt(w, h, spp, flags=POOL, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, num_bounces=8, flags=flags, **kw)


@lru_cache(maxsize=None)
def _three(w, h):
    return scene_data("three_spheres", w, h)


_REFS = {}


def _want_image(oracle, key, sd, **kw):
    """The oracle's image of a case, computed once per session and never written to."""
    if key not in _REFS:
        img = oracle.render(sd, _pt(flags=0, **kw))
        img.setflags(write=False)
        _REFS[key] = img
    return _REFS[key]


def _check_image(ctx, oracle, sd, what, kernel=DEFAULT_BUILD, flags=POOL, **kw):
    ctx.set_scene(sd)
    got = ctx.render(_pt(flags=flags, **kw))
    assert ctx.last_kernel().startswith(kernel), (what, ctx.last_kernel())
    assert_images_equal(got, _want_image(oracle, (what, tuple(sorted(kw.items()))), sd, **kw), what)


def _check_sums(ctx, oracle, sd, what, kernel=DEFAULT_BUILD, flags=POOL, **kw):
    ctx.set_scene(sd)
    p = _pt(flags=flags, **kw)
    ctx.accum_reset(p)
    ctx.accum_add(p)
    got = ctx.accum_read(p)
    assert ctx.last_kernel().startswith(kernel), (what, ctx.last_kernel())
    want = oracle.render_pt_sums(sd, _pt(flags=0, **kw))
    assert np.array_equal(got, want), f"{what}: {int((got != want).any(-1).sum())} of {got.shape[0] * got.shape[1]} pixels differ"


@pytest.mark.parametrize("sample_begin", [ENTRIES - 20, 0, ENTRIES - SPP, ENTRIES, 0xFFFFFFFF - SPP],
                         ids=["65516", "zero", "65496", "65536", "last-index"])
def test_first_sample_indices(gpu_ctx, oracle, sample_begin):
    """Samples 65 516 .. 65 555, 0 .. 39, 65 496 .. 65 535, 65 536 .. 65 575, and the 40 that end at 0xFFFFFFFE: sample + 1 = 0xFFFFFFFF."""
    _check_image(gpu_ctx, oracle, _three(W, H), "first sample", w=W, h=H, spp=SPP, sample_begin=sample_begin)


def test_wrapping_launch_is_refused_by_library_and_oracle(gpu_ctx, oracle):
    sd = _three(W, H)
    gpu_ctx.set_scene(sd)
    p = _pt(W, H, SPP, sample_begin=0xFFFFFFF0)
    with pytest.raises(m.MirtError) as e:
        gpu_ctx.render(p)
    assert e.value.status == _abi.MIRT_ERR_SPP_RANGE
    assert oracle.render_status(sd.as_c(), p) == _abi.MIRT_ERR_SPP_RANGE


def test_narrow_strips_span_samples(gpu_ctx, oracle):
    """130 spp on a small frame: every strip is 4 pixels wide (the end-of-frame level), so the 64 lanes of a GEN step hold 16
    different samples of 4 records."""
    _check_image(gpu_ctx, oracle, _three(20, 6), "4-pixel strips", w=20, h=6, spp=130, sample_begin=ENTRIES - 70)


def test_seed(gpu_ctx, oracle):
    _check_sums(gpu_ctx, oracle, _three(W, H), "seed", w=W, h=H, spp=SPP, seed=0x0123456789ABCDEF)
    _check_image(gpu_ctx, oracle, _three(W, H), "seed, across the end", w=W, h=H, spp=SPP, seed=7, sample_begin=ENTRIES - 20)


@pytest.mark.parametrize("w,h", [(40, 7), (5, 9), (37, 5)], ids=["w40-wraps-rows", "w5-narrow-path", "w37-ragged-9"])
def test_strip_shapes(gpu_ctx, oracle, w, h):
    """Width 40: a 16-pixel strip wraps into the next row; width 5: the addressing of frames narrower than a strip (a strip spans
    four rows); 280, 45 and 185 pixels all leave a ragged last strip (8, 13, 9 pixels)."""
    _check_sums(gpu_ctx, oracle, _three(w, h), f"{w}x{h}", w=w, h=h, spp=SPP, seed=3)


def test_bands_and_tile_partitions(gpu_ctx, oracle):
    sd = _three(W, H)
    _check_image(gpu_ctx, oracle, sd, "band", w=W, h=H, spp=SPP, row_begin=3, row_end=17)
    _check_image(gpu_ctx, oracle, sd, "band of narrow rows", w=W, h=H, spp=SPP, row_begin=19, row_end=20)
    for part in range(3):
        _check_image(gpu_ctx, oracle, sd, f"part {part} of 3", w=W, h=H, spp=SPP, tile_rows=4, n_parts=3, part=part, seed=5)
    sd5 = _three(5, 20)
    for part in range(3):                        # the narrow path goes through abs_row for every pixel
        _check_image(gpu_ctx, oracle, sd5, f"width 5, part {part} of 3", w=5, h=20, spp=SPP, tile_rows=4, n_parts=3, part=part)


def test_tile_build(gpu_ctx, oracle):
    w, h = 40, 12
    _check_image(gpu_ctx, oracle, scene_data("earth", w, h), "tile build", kernel="render_pt_pool_tile_kernel<256,112,6,false,false,",
                 flags=POOL | m.MIRT_FLAG_TEXEL_TILES, w=w, h=h, spp=SPP, sample_begin=ENTRIES - 20)


def test_progressive_frame_build(gpu_ctx, oracle):
    """Two fused frames of 17 + 23 samples: the second starts at sample 17 of every pixel."""
    sd = _three(W, H)
    gpu_ctx.set_scene(sd)
    gpu_ctx.accum_reset(_pt(W, H, 17))
    for spp in (17, 23):
        img = gpu_ctx.accum_frame(_pt(W, H, spp))
        assert gpu_ctx.last_kernel().startswith("render_pt_pool_frame_kernel<256,112,6,false,false,3,"), gpu_ctx.last_kernel()
    assert np.array_equal(gpu_ctx.accum_read(_pt(W, H, 23)), oracle.render_pt_sums(sd, _pt(W, H, SPP, flags=0)))
    assert_images_equal(img, _want_image(oracle, ("frames",), sd, w=W, h=H, spp=SPP), "progressive frames")


def test_grid_build(gpu_ctx, oracle):
    """A 40-sphere soup: the pooled kernel's grid build."""
    w, h = 40, 12
    cen, rad = sphere_soup(np.random.default_rng(31), 37, 2.5, 0.1, 0.35)
    assert len(rad) == 40
    mat = np.random.default_rng(32).integers(0, 6, len(rad))
    sd = soup_scene(cen, rad, mat, look(w, h, (6.0, 2.0, 5.0), (0.0, 0.5, 0.0), vfov=40.0, focus=8.0))
    _check_image(gpu_ctx, oracle, sd, "grid build", kernel="render_pt_pool_kernel<1024,", w=w, h=h, spp=SPP, sample_begin=ENTRIES - 20)
    assert ",true," in gpu_ctx.last_kernel() or gpu_ctx.last_kernel().endswith(",true>"), gpu_ctx.last_kernel()


def test_counting_build(gpu_ctx, oracle):
    sd = _three(W, H)
    gpu_ctx.set_scene(sd)
    p = _pt(W, H, SPP, flags=POOL | m.MIRT_FLAG_COUNT_WORK, sample_begin=ENTRIES - 20)
    got = gpu_ctx.render(p)
    gs = gpu_ctx.stats()
    assert gpu_ctx.last_kernel().startswith("render_pt_pool_kernel<256,112,1,true,false,5,"), gpu_ctx.last_kernel()
    want = oracle.render(sd, p)
    os_ = oracle.stats()
    assert_images_equal(got, want, "counting build")
    assert {k: gs[k] for k in COUNTERS} == {k: os_[k] for k in COUNTERS}


def test_two_contexts_on_one_device(gpu_ctx, oracle):
    """A second context on the device renders the same frame; closing it leaves the first one's launches as they were."""
    sd = _three(W, H)
    kw = dict(w=W, h=H, spp=SPP, sample_begin=ENTRIES - 20)
    other = m.Context(0)
    try:
        _check_image(other, oracle, sd, "first sample", **kw)
        _check_image(gpu_ctx, oracle, sd, "first sample", **kw)
    finally:
        other.close()
    _check_image(gpu_ctx, oracle, sd, "first sample", **kw)
