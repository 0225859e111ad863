"""MIRT_SCENE_HBM: worlds beyond the LDS budget, with the scene's tables in device memory and the nearest hit through a BVH.

The BVH build must give the flat scan's image byte for byte (min f, ties to the lower index): against the LDS builds
on scenes that fit them, against the oracle beyond them, and against the device's own flat scan (MIRT_FLAG_NO_GRID) at sizes the
oracle cannot reach."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from helpers import assert_images_equal, bimodal_soup, scene_data
from hbm_worlds import clustered_soup, field_materials, look, rtiow_field, scene_from_arrays, sphere_array

pytestmark = pytest.mark.gpu

PT = m.MIRT_MODE_PT
COUNTERS = ("rays", "sphere_tests", "roots", "hits", "scatter", "sky_misses")


def _pt(w, h, spp, **kw):
    kw.setdefault("num_bounces", 8)
    return m.make_params(w, h, spp, mode=PT, **kw)


@pytest.fixture(scope="module")
def hctx():
    ctx = m.Context(0)
    yield ctx
    ctx.close()


def _hbm_kernel(ctx):
    return ctx.last_kernel()


def _random_soup(n, seed, w, h):
    rng = np.random.default_rng(seed)
    cen = rng.uniform(-4, 4, (n, 3))
    cen[:, 2] -= 6
    rad = rng.uniform(0.05, 0.6, n) * (1.0 if n < 200 else 0.4)
    mats, tex = field_materials()
    arr = sphere_array(cen, rad, rng.integers(0, len(mats), n))
    return scene_from_arrays(look(w, h, (0, 0.5, 4), (0, 0, -6), vfov=50), arr, mats, tex)


def _lds_scenes(w, h):
    out = [(name, scene_data(name, w, h)) for name in ("three_spheres", "main_rs_scene", "earth", "rtiow_final")]
    cs, rs = bimodal_soup()
    mats, tex = field_materials()
    rng = np.random.default_rng(5)
    arr = sphere_array(cs, rs, rng.integers(0, len(mats), len(rs)))
    out.append(("bimodal_soup", scene_from_arrays(look(w, h, (0, 0, 3), (0, 0, 0), vfov=40), arr, mats, tex)))
    for n, seed in ((32, 1), (500, 2), (3000, 3)):
        out.append((f"soup{n}", _random_soup(n, seed, w, h)))
    return out


# 1. the HBM build equals the LDS builds, byte for byte (images and accumulated sums), at every LDS schedule's sample count
def test_hbm_equals_lds_builds(hctx):
    w, h = 64, 40
    for name, sd in _lds_scenes(w, h):
        for spp in (1, 2, 8, 32):
            p = _pt(w, h, spp)
            hctx.set_scene(sd)
            want = hctx.render(p)
            lds_kernel = hctx.last_kernel()
            hctx.set_scene(sd, hbm=True)
            got = hctx.render(p)
            assert hctx.last_kernel() == "render_pt_hbm_kernel<false,false,true,true>", hctx.last_kernel()
            assert_images_equal(got, want, f"{name} spp{spp} against {lds_kernel}")
        # accumulated exact sums
        p = _pt(w, h, 4)
        sums = []
        for hbm in (False, True):
            hctx.set_scene(sd, hbm=hbm)
            hctx.accum_reset(p)
            hctx.accum_add(p)
            sums.append(hctx.accum_read(p))
        assert np.array_equal(sums[0], sums[1]), f"{name}: accumulated sums differ"


def test_hbm_hosek_sky_and_frame_stream(hctx):
    w, h = 48, 32
    sd = scene_data("rtiow_final", w, h)
    sky = _abi.MirtSkyState()
    for c in range(3):
        for i, v in enumerate([-1.1, -0.3, 0.5, 1.2, -2.5, 0.4, 0.2, 1.5, 0.6]):
            sky.params[9 * c + i] = v * (1.0 + 0.1 * c)
        sky.radiances[c] = 1.0 + c
    sky.sun_direction[:] = [0.0, 0.6, 0.8, 0.0]
    sd.sky = sky
    for p in (_pt(w, h, 8, flags=m.MIRT_FLAG_SKY_HOSEK), _pt(w, h, 8, frame_spp=2, frame_begin=3)):
        hctx.set_scene(sd)
        want = hctx.render(p)
        hctx.set_scene(sd, hbm=True)
        assert_images_equal(hctx.render(p), want, f"flags {p.flags} frame_spp {p.frame_spp}")


# 2. beyond LDS, against the oracle: images and exact 64-bit sums
@pytest.mark.parametrize("n,kind", [(5000, "field"), (20000, "field"), (20000, "soup"), (100000, "field")])
def test_beyond_lds_against_oracle(hctx, oracle, n, kind):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(n) if kind == "field" else clustered_soup(n)
    cam = look(w, h, (13, 2, 3), (0, 0, 0), vfov=25, aperture=0.05) if kind == "field" else look(w, h, (0, 5, 60), (0, 0, 0), vfov=60)
    sd = scene_from_arrays(cam, arr, mats, tex)
    p = _pt(w, h, 4, num_bounces=6 if n < 100000 else 4)
    hctx.set_scene(sd, hbm=True)
    got = hctx.render(p)
    assert_images_equal(got, oracle.render(sd, p), f"{kind} {n}")
    hctx.accum_reset(p)
    hctx.accum_add(p)
    assert np.array_equal(hctx.accum_read(p), oracle.render_pt_sums(sd, p)), f"{kind} {n}: sums"


# 3. BVH against the device's flat scan of the same tables (MIRT_FLAG_NO_GRID)
@pytest.mark.parametrize("n,w,h,spp,band", [(20000, 256, 144, 8, None), (100000, 256, 144, 8, None), (1000000, 128, 72, 2, (24, 48))])
def test_bvh_against_device_flat_scan(hctx, n, w, h, spp, band):
    arr, mats, tex = rtiow_field(n, seed=n)
    sd = scene_from_arrays(look(w, h, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    rows = dict(row_begin=band[0], row_end=band[1]) if band else {}
    got = hctx.render(_pt(w, h, spp, num_bounces=4, **rows))
    assert hctx.last_kernel() == "render_pt_hbm_kernel<false,false,true,true>"
    flat = hctx.render(_pt(w, h, spp, num_bounces=4, flags=m.MIRT_FLAG_NO_GRID, **rows))
    assert hctx.last_kernel().startswith("render_pt_hbm_kernel<false,false,false,")
    assert_images_equal(got, flat, f"{n} spheres: BVH vs flat scan")


# 4. adversarial geometry, against the flat scan and the oracle
def _adversarial():
    """The worlds of tests/grid_rounding.py::adversarial_worlds at their HBM size: 1 000 copies of one sphere (the lowest index must
    win), a tangent 13^3 lattice seen along an axis and obliquely, a camera inside a big sphere, and rays grazing r = 1e-3 spheres at
    distance 1e3 with zero-radius and non-finite spheres among them.  The LDS grid builds are held to the same definitions
    (test_gpu_grid_rounding.py)."""
    from grid_rounding import adversarial_worlds
    mats, tex = field_materials()
    return [(name, sphere_array(cen, rad, mat), eye, at, vfov) for name, cen, rad, mat, eye, at, vfov in adversarial_worlds(lattice_half=6)], mats, tex


@pytest.mark.parametrize("case", range(5))
def test_adversarial_geometry(hctx, oracle, case):
    cases, mats, tex = _adversarial()
    name, arr, eye, at, vfov = cases[case]
    w, h = 48, 32
    sd = scene_from_arrays(look(w, h, eye, at, vfov=vfov), arr, mats, tex)
    p = _pt(w, h, 4, num_bounces=5)
    hctx.set_scene(sd, hbm=True)
    got = hctx.render(p)
    assert_images_equal(got, hctx.render(_pt(w, h, 4, num_bounces=5, flags=m.MIRT_FLAG_NO_GRID)), f"{name}: BVH vs flat scan")
    assert_images_equal(got, oracle.render(sd, p), f"{name}: BVH vs oracle")


# 5. parity mode on an HBM world, with its counters
@pytest.mark.parametrize("spp", [2, 21])
def test_parity_mode(hctx, oracle, spp):
    w, h = 80, 60
    arr, mats, tex = rtiow_field(10000, seed=3)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    p = m.make_params(w, h, spp, flags=m.MIRT_FLAG_COUNT_WORK)
    got = hctx.render(p)
    assert hctx.last_kernel().startswith("render_parity_hbm_kernel<true,")
    gs = hctx.stats()
    assert_images_equal(got, oracle.render(sd, p), f"parity spp{spp}")
    os_ = oracle.stats()
    assert {k: gs[k] for k in COUNTERS} == {k: os_[k] for k in COUNTERS}
    assert_images_equal(hctx.render(m.make_params(w, h, spp)), got, "plain parity build")


# 6. counting: the BVH build's counters; gates on the tree's quality
def test_counting(hctx, oracle):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(20000, seed=4)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    p = _pt(w, h, 4, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID)
    got = hctx.render(p)
    gs = hctx.stats()
    assert_images_equal(got, oracle.render(sd, p), "counting BVH build")
    os_ = oracle.stats()
    for k in ("rays", "hits", "scatter", "sky_misses"):
        assert gs[k] == os_[k], k
    assert gs["sphere_tests"] < 0.01 * os_["sphere_tests"]
    assert gs["grid_cells"] > 0
    # the flat scan's counting build counts exactly the oracle's work
    p = _pt(w, h, 4, flags=m.MIRT_FLAG_COUNT_WORK)
    assert_images_equal(hctx.render(p), got, "counting flat build")
    gs = hctx.stats()
    assert {k: gs[k] for k in COUNTERS} == {k: os_[k] for k in COUNTERS}


def test_million_sphere_tree_quality(hctx):
    w, h = 128, 72
    arr, mats, tex = rtiow_field(1000000, seed=7)
    sd = scene_from_arrays(look(w, h, (40, 6, 30), (0, 0, 0), vfov=35), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    hctx.render(_pt(w, h, 2, flags=m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_COUNT_GRID))
    gs = hctx.stats()
    assert gs["sphere_tests"] / gs["rays"] <= 64, gs
    assert gs["grid_cells"] / gs["rays"] <= 256, gs


# 7. accumulation
def test_accumulation(hctx, oracle):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(6000, seed=6)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    p2, p8 = _pt(w, h, 2), _pt(w, h, 8)
    hctx.accum_reset(p2)
    for _ in range(4):
        hctx.accum_add(p2)
    assert hctx.accum_samples() == 8
    assert_images_equal(hctx.accum_resolve(p8), hctx.render(p8), "4 x 2 spp vs 8 spp")
    assert np.array_equal(hctx.accum_read(p8), oracle.render_pt_sums(sd, p8))


# 8. bands, tile interleave, node loopback
def test_bands_tiles_and_node(hctx):
    w, h = 64, 48
    arr, mats, tex = rtiow_field(8000, seed=8)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    hctx.set_scene(sd, hbm=True)
    full = hctx.render(_pt(w, h, 4))
    band = hctx.render(_pt(w, h, 4, row_begin=10, row_end=30))
    assert_images_equal(band, full[10:30], "band")
    img = np.zeros_like(full)
    for part in range(3):
        p = _pt(w, h, 4, tile_rows=4, n_parts=3, part=part)
        out = hctx.render(p)
        for i in range(out.shape[0]):
            img[m.params_out_row_index(p, i)] = out[i]
    assert_images_equal(img, full, "tile interleave")
    for n in (2, 4):
        node = m.Node([0] * n)
        node.set_scene(sd, hbm=True)
        assert_images_equal(node.render(_pt(w, h, 4)), full, f"node of {n}")
        node.close()


# 9. API
def test_api(hctx):
    w, h = 48, 32
    sd = scene_data("rtiow_final", w, h)
    p = _pt(w, h, 4)
    hctx.set_scene(sd)
    want, kname = hctx.render(p), hctx.last_kernel()
    c = sd.as_c()
    assert m.lib().mirt_ctx_set_scene_ex(hctx._h, C.byref(c), 0) == 0
    assert_images_equal(hctx.render(p), want, "flags = 0")
    assert hctx.last_kernel() == kname
    # unknown bits; a refused call leaves the scene in place
    assert m.lib().mirt_ctx_set_scene_ex(hctx._h, C.byref(c), 2) == _abi.MIRT_ERR_BAD_MODE
    assert m.lib().mirt_ctx_set_scene_ex(hctx._h, C.byref(c), _abi.MIRT_SCENE_HBM | 4) == _abi.MIRT_ERR_BAD_MODE
    too_many = _abi.MirtScene()
    too_many.camera = c.camera
    too_many.n_spheres = _abi.MIRT_SCENE_HBM_MAX_SPHERES + 1
    too_many.spheres = C.cast(C.c_void_p(16), C.POINTER(_abi.MirtSphere))     # never read: the count is refused first
    assert m.lib().mirt_ctx_set_scene_ex(hctx._h, C.byref(too_many), _abi.MIRT_SCENE_HBM) == _abi.MIRT_ERR_SCENE_TOO_LARGE
    assert_images_equal(hctx.render(p), want, "after refused calls")
    assert hctx.last_kernel() == kname
    # the 5 000-sphere world test_gpu_api.py shows refused by mirt_ctx_set_scene renders through MIRT_SCENE_HBM
    cam = look(8, 8, (0, 0, 3), (0, 0, -1), vfov=60)
    mats, tex = m.flatten_materials([m.Material.Dielectric(1.5)] * 3)
    many = m.SceneData(cam, [m.Sphere.new((0, 0, -5), 0.1, 0).to_c()] * 5000, mats, tex)
    with pytest.raises(m.MirtError):
        hctx.set_scene(many)
    hctx.set_scene(many, hbm=True)
    assert hctx.render(_pt(8, 8, 2)).shape == (8, 8, 4)
    # LDS and HBM scenes alternating on one context
    for hbm in (False, True, False, True):
        hctx.set_scene(sd, hbm=hbm)
        assert_images_equal(hctx.render(p), want, f"alternating hbm={hbm}")


# 10. the reference's host objects take a world beyond LDS
def test_python_raytracer_and_layer(oracle):
    w, h = 48, 32
    arr, _, _ = rtiow_field(20000, seed=10)
    mats = [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))),
            m.Material.Dielectric(refraction_index=1.5),
            m.Material.Metal(albedo=m.Texture.new_from_color((0.7, 0.6, 0.5)), fuzz=0.3)]   # layer.rs reads material_data[2]'s texture
    spheres = [m.Sphere.new(tuple(map(float, s["center"][:3])), float(s["radius"]), int(s["material_idx"]) % 3) for s in arr]
    rp = m.RenderParams(camera=m.FlyCameraController.default().renderer_camera(), viewport_size=(w, h),
                        sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=4, num_bounces=4))
    rt = m.Raytracer(m.Scene(spheres, mats), rp, device=0)
    got = rt.render()
    want = oracle.render(rt.scene_data(), m.make_params(w, h, 4, mode=PT, num_bounces=4))
    assert_images_equal(got, want, "Raytracer, 20 000 spheres")
    rt.close()
    layer = m.Layer.new([w, h], rp, scene=m.Scene(spheres, mats))
    layer.set_global_data()
    layer.set_data(rp)
    want = oracle.render(layer.scene_data(), m.make_params(w, h, 4))
    assert_images_equal(layer.register_texture(), want, "Layer, 20 000 spheres")
    layer.close()


# 11. the fast-math build of the BVH kernel
def test_fast_math(hctx):
    w, h = 480, 270
    sd = scene_data("rtiow_final", w, h)
    hctx.set_scene(sd, hbm=True)
    exact = hctx.render(_pt(w, h, 64))
    p = _pt(w, h, 64, flags=m.MIRT_FLAG_FAST_MATH)
    fast = hctx.render(p)
    assert hctx.last_kernel() == "fast_build::render_pt_hbm_kernel<false,false,true,true>"
    assert np.array_equal(fast, hctx.render(p)), "fast build is not deterministic"
    d = np.abs(fast.astype(np.int32) - exact.astype(np.int32)).max(axis=2)
    assert (d <= 1).mean() >= 0.999, f"{(d <= 1).mean():.5f} of the pixels within 1"
