"""mirt_ctx_render_features, mirt_ctx_render_features_device and mirt_camera_pixel_ray through the layers that need no device: the
library's exports and its checks before any HIP call, the ctypes mirror's layout, the Rust crate's source, the Python wrappers'
argument checks, the host restatement of the centre ray -- and an audit, on the CPU reference alone, that the fixture of
tests/test_gpu_features.py shows every shading routine, the image texture and the sky."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, FEATURE_DTYPE, RAY_DTYPE
import feature_ref as fr
import hbm_worlds

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
NEW = {"mirt_ctx_render_features": 5, "mirt_ctx_render_features_device": 6, "mirt_camera_pixel_ray": 6}
f32 = np.float32


def test_the_library_exports_the_three_symbols():
    lib = m.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.SYMBOLS, name


def test_header_ctypes_and_rust_agree_on_arity():
    for name, arity in NEW.items():
        h = re.search(r"^int %s\s*\(([^)]*)\)\s*;" % name, HEADER, re.M)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, RS)
        assert h and r, name
        count = lambda args: len([a for a in args.split(",") if a.strip()])
        assert count(h.group(1)) == count(r.group(1)) == len(_abi.SYMBOLS[name][1]) == arity, name
        assert _abi.SYMBOLS[name][0] is C.c_int


def test_struct_size_offsets_and_field_order():
    F = _abi.MirtFeaturePixel
    assert C.sizeof(F) == 32
    assert (F.albedo.offset, F.t.offset, F.normal.offset, F.sphere.offset) == (0, 12, 16, 28)
    assert FEATURE_DTYPE.itemsize == 32 and [FEATURE_DTYPE.fields[f][1] for f in ("albedo", "t", "normal", "sphere")] == [0, 12, 16, 28]
    assert m.FEATURE_DTYPE is FEATURE_DTYPE
    py = [f for f, _ in F._fields_]
    body = re.search(r"typedef struct MirtFeaturePixel\s*\{(.*?)\}\s*MirtFeaturePixel;", HEADER, re.S).group(1)
    in_header = [w for decl in body.split(";") if decl.strip() for w in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", re.sub(r"^\s*\w+\s+", "", decl.strip()))]
    assert in_header == py, in_header
    rust = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct MirtFeaturePixel \{(.*?)\n\}", RS, re.S)
    assert rust and re.findall(r"pub (\w+):", rust.group(1)) == py
    assert HEADER.count("sizeof(MirtFeaturePixel) == 32") == 2           # static_assert and _Static_assert


def test_constants_match_the_header_and_the_crate():
    assert re.search(r"enum \{ MIRT_FEATURES_FLAT = 1u << 0 \};", HEADER)
    assert re.search(r"pub const MIRT_FEATURES_FLAT: u32 = 1 << 0;", RS)
    assert _abi.MIRT_FEATURES_FLAT == 1 == m.MIRT_FEATURES_FLAT
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0    # a new capability, no new version, no new status code
    assert "MIRT_ERR_FEATURE" not in HEADER


def test_a_null_context_and_bad_flags_are_refused_before_any_device_call():
    lib = m.lib()
    p = m.make_params(4, 2, 0)
    out = np.zeros(8, FEATURE_DTYPE)
    po = C.c_void_p(out.ctypes.data)
    for flags in (0, _abi.MIRT_FEATURES_FLAT, 2, 3, 0xFFFFFFFF):
        for params, o, n in ((C.byref(p), po, out.nbytes), (None, po, out.nbytes), (C.byref(p), None, out.nbytes), (C.byref(p), po, 0)):
            assert lib.mirt_ctx_render_features(None, params, flags, o, n) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_render_features_device(None, params, flags, o, n, None) == _abi.MIRT_ERR_NULL_POINTER
    assert b"ctx" in lib.mirt_last_error()
    assert not out.view(np.uint8).any()


# ---- the Python wrappers' argument checks, against a context that does not exist ----

class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("params", [None, (67, 45, 0), np.zeros(1, FEATURE_DTYPE), np.zeros((45, 67), np.float32), {"width": 67}, "params"],
                         ids=["None", "tuple", "records", "f32 [h, w]", "dict", "str"])
def test_the_wrappers_refuse_params_that_are_no_params(params, no_library):
    with pytest.raises(ValueError):
        Context.render_features(_NoLibrary(), params)
    with pytest.raises(ValueError):
        Context.render_features_device(_NoLibrary(), params, 0x1000, 32)


@pytest.mark.parametrize("flat", [1, 0, None, "flat", 1.0, _abi.MIRT_FEATURES_FLAT])
def test_the_wrappers_refuse_a_flat_that_is_no_bool(flat, no_library):
    p = m.make_params(4, 2, 0)
    with pytest.raises(ValueError):
        Context.render_features(_NoLibrary(), p, flat)
    with pytest.raises(ValueError):
        Context.render_features_device(_NoLibrary(), p, 0x1000, 256, flat)


@pytest.mark.parametrize("d_ptr, nbytes", [(0, 256), (-8, 256), (None, 256), (1.0, 256), (True, 256), (np.zeros(8, FEATURE_DTYPE), 256),
                                             (0x1000, -1), (0x1000, 1.5), (0x1000, None), (0x1000, True)])
def test_render_features_device_refuses_pointers_that_are_no_addresses_and_sizes_that_are_no_counts(d_ptr, nbytes, no_library):
    with pytest.raises(ValueError):
        Context.render_features_device(_NoLibrary(), m.make_params(4, 2, 0), d_ptr, nbytes)


@pytest.mark.parametrize("args", [(None, 4, 4, 0, 0), ("camera", 4, 4, 0, 0), (np.zeros(24, np.float32), 4, 4, 0, 0), ("cam", 4.0, 4, 0, 0), ("cam", 4, 4, -1, 0),
                                  ("cam", 4, 4, 0, 1.5), ("cam", 4, 4, True, 0), ("cam", 2 ** 32, 4, 0, 0)])
def test_camera_pixel_ray_refuses_wrong_types_before_the_library(args, no_library):
    cam = fr.fixture_camera() if isinstance(args[0], str) and args[0] == "cam" else args[0]
    with pytest.raises(ValueError):
        m.camera_pixel_ray(cam, *args[1:])


# ---- mirt_camera_pixel_ray ----

def _formula(cam, w, h, x, y):
    """The centre ray in float32 with fmaf, written out: what include/mirt.h states."""
    from grid_rounding import fma32
    inv_w, inv_h = f32(1.0) / f32(w), f32(1.0) / f32(h)
    u = np.array([(f32(x) + f32(0.5)) * inv_w], f32)
    v = np.array([f32(1.0) - (f32(y) + f32(0.5)) * inv_h], f32)
    eye, hor, ver, llc = (np.asarray(a[:3], f32) for a in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    d = [(fma32(v, ver[k:k + 1], fma32(u, hor[k:k + 1], llc[k:k + 1]))[0] - eye[k]).astype(f32) for k in range(3)]
    return eye, np.array(d, f32)


@pytest.mark.parametrize("aperture", [0.0, 0.2], ids=["pinhole", "lens"])
def test_camera_pixel_ray_is_the_float32_fmaf_formula_bit_for_bit(aperture):
    cam = fr.fixture_camera(aperture)
    assert (cam.lens_radius != 0) == (aperture != 0)
    ys, xs = np.divmod(np.arange(fr.W * fr.H), fr.W)
    ro, rd = fr.centre_rays(cam, fr.W, fr.H, xs, ys)                   # the reference's rays: the same formula, vectorised
    got = np.concatenate([m.camera_pixel_ray(cam, fr.W, fr.H, int(x), int(y)) for x, y in zip(xs, ys)])
    assert got.dtype == RAY_DTYPE and got.shape == (fr.W * fr.H,)
    assert np.array_equal(got["origin"].view(np.uint32), ro.view(np.uint32)), "the lens is ignored: origin = eye"
    assert np.array_equal(got["direction"].view(np.uint32), rd.view(np.uint32))
    assert (got["t_max"] == 1000.0).all() and not got["_pad"].view(np.uint32).any()
    for x, y in ((0, 0), (66, 44), (31, 17)):                          # and against the formula written out pixel by pixel
        eye, d = _formula(cam, fr.W, fr.H, x, y)
        r = got[y * fr.W + x]
        assert np.array_equal(r["origin"].view(np.uint32), eye.view(np.uint32)) and np.array_equal(r["direction"].view(np.uint32), d.view(np.uint32))


def test_camera_pixel_ray_error_codes():
    lib = m.lib()
    cam, ray = fr.fixture_camera(), _abi.MirtRay()
    assert lib.mirt_camera_pixel_ray(None, 4, 4, 0, 0, C.byref(ray)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_camera_pixel_ray(C.byref(cam), 4, 4, 0, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    for w, h in ((0, 4), (4, 0), (0, 0)):
        assert lib.mirt_camera_pixel_ray(C.byref(cam), w, h, 0, 0, C.byref(ray)) == _abi.MIRT_ERR_VIEWPORT_SIZE
    for x, y in ((4, 0), (0, 4), (0xFFFFFFFF, 0), (4, 4)):
        assert lib.mirt_camera_pixel_ray(C.byref(cam), 4, 4, x, y, C.byref(ray)) == _abi.MIRT_ERR_BAD_ROWS
    assert lib.mirt_camera_pixel_ray(C.byref(cam), 4, 4, 3, 3, C.byref(ray)) == 0 and ray.t_max == 1000.0
    with pytest.raises(m.MirtError) as e:
        m.camera_pixel_ray(cam, 4, 4, 4, 0)
    assert e.value.status == _abi.MIRT_ERR_BAD_ROWS
    # Python's pixel_ray keeps its own (float64, dividing) arithmetic: the two agree to rounding, not to the bit
    o, d = m.pixel_ray(cam, 67, 45, 31, 17)
    r = m.camera_pixel_ray(cam, 67, 45, 31, 17)[0]
    assert np.array_equal(o, r["origin"]) and np.allclose(d, r["direction"], rtol=0, atol=4e-6 * np.abs(d).max())


# ---- the fixture is not vacuous: asserted on the CPU reference alone ----

def test_the_fixture_shows_every_routine_the_image_texture_and_the_sky():
    ref = fr.fixture()
    centre = ref.layer()
    arr, mats = ref.arr, ref.mats
    hit = centre["hit"]
    assert len(arr) == 3000 and hit.shape == (67 * 45,)
    # audited: 908 misses; lambertian 278, metal 440, glass 109, checkerboard 1258, missing material 22 pixels; 143 pixels on the
    # image-textured material; 120 distinct winning spheres
    assert (~hit).sum() >= 500
    midx = arr["material_idx"][centre["hits"]["sphere"][hit]]
    routine = np.minimum(np.array([mats[int(k)].id for k in midx]), 4)
    census = np.bincount(routine, minlength=5)
    print("misses", int((~hit).sum()), "routines", census.tolist(), "image", int((midx == fr.IMAGE_MATERIAL).sum()),
          "winners", len(np.unique(centre["hits"]["sphere"][hit])))
    assert (census >= 20).all(), census
    assert mats[fr.IMAGE_MATERIAL].desc1.width > 1 and (midx == fr.IMAGE_MATERIAL).sum() >= 100
    assert len(np.unique(centre["hits"]["sphere"][hit])) >= 50
    frame = ref.frame(0)
    assert frame.shape == (45, 67) and np.isfinite(frame["normal"]).all() and (frame["t"].ravel()[~hit] == 0).all()
    on_image = frame["albedo"].reshape(-1, 3)[hit][midx == fr.IMAGE_MATERIAL]
    assert len(np.unique(on_image, axis=0)) >= 50                       # the image texture really varies over its pixels
    # jittered samples differ from the centre rays, and a seed changes them
    (o0, d0), (oa, da), (_, db), (_, dc) = ref.rays(), ref.rays(0, 0), ref.rays(0, 9), ref.rays(5, 0)
    assert not np.array_equal(da, d0) and not np.array_equal(da, db) and not np.array_equal(da, dc)
    assert np.array_equal(oa, o0)                                       # a pinhole camera: every ray starts at the eye
    lens = fr.fixture(0.2)
    assert not fr.is_pinhole(lens.cam) and fr.is_pinhole(ref.cam)
    assert not np.array_equal(lens.rays(0, 0)[0], o0) and np.array_equal(lens.rays()[0], o0)


def test_the_reference_accumulates_in_sample_order_and_divides_once():
    ref = fr.fixture()
    one, three = ref.frame(1), ref.frame(3)
    l0, l1, l2 = (ref.layer(s, 0) for s in range(3))
    assert np.array_equal(one["sphere"], three["sphere"]) and np.array_equal(one["t"], three["t"])     # the centre ray's, whatever spp
    all3 = l0["hit"] & l1["hit"] & l2["hit"]
    with np.errstate(all="ignore"):
        want = (((l0["hits"]["normal"] + l1["hits"]["normal"]).astype(f32) + l2["hits"]["normal"]).astype(f32) / f32(3.0)).astype(f32)
    assert all3.sum() > 1000 and np.array_equal(three["normal"].reshape(-1, 3)[all3], want[all3])
    none = ~(l0["hit"] | l1["hit"] | l2["hit"])
    assert none.sum() > 300 and not three["normal"].reshape(-1, 3)[none].any() and not three["albedo"].reshape(-1, 3)[none].any()
    part = m.make_params(67, 45, 0, tile_rows=4, n_parts=3, part=1)
    rows = [m.params_out_row_index(part, i) for i in range(m.params_out_rows(part))]
    assert rows[:5] == [4, 5, 6, 7, 16] and fr.same_bits(ref.of(part), ref.frame(0)[rows]).all()
