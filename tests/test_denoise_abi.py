"""mirt_ctx_denoise and mirt_ctx_denoise_device through the layers that need no device: the library's exports and its first check, the
ctypes mirror's layout, the Rust crate's and the C++ mirror's source, the Python wrappers' argument checks -- and, on the CPU reference
alone, the two restatements of the rule against each other and the one condition on quality the feature is held to: on three_spheres
the filtered frame is closer to a many-sample frame than the raw one."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, FEATURE_DTYPE
import denoise_ref as dr
import feature_ref as fr
import hbm_worlds
import oracle_binding as ob

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
NEW = {"mirt_ctx_denoise": 7, "mirt_ctx_denoise_device": 8}
f32 = np.float32


# ---- the ABI ----

def test_the_library_exports_the_two_symbols():
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
        assert re.search(r"\b%s\(ctx," % name, HPP), f"the C++ mirror does not call {name}"


def test_struct_size_offsets_and_field_order():
    D = _abi.MirtDenoiseParams
    assert C.sizeof(D) == 32
    assert (D.source.offset, D.levels.offset, D.normal_log2.offset, D.flags.offset, D.sigma_colour.offset, D._pad.offset) == (0, 4, 8, 12, 16, 20)
    py = [f for f, _ in D._fields_]
    body = re.search(r"typedef struct MirtDenoiseParams\s*\{(.*?)\}\s*MirtDenoiseParams;", HEADER, re.S).group(1)
    in_header = [w for decl in body.split(";") if decl.strip() for w in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", re.sub(r"^\s*\w+\s+", "", decl.strip()))]
    assert in_header == py, in_header
    rust = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct MirtDenoiseParams \{(.*?)\n\}", RS, re.S)
    assert rust and re.findall(r"pub (\w+):", rust.group(1)) == py
    assert re.findall(r"pub \w+: ([^,\n]+),", rust.group(1)) == ["u32", "u32", "u32", "u32", "f32", "[u32; 3]"]
    assert HEADER.count("sizeof(MirtDenoiseParams) == 32") == 2         # static_assert and _Static_assert
    assert "sizeof(MirtDenoiseParams) == 32" in HPP


def test_constants_match_the_header_and_the_crate():
    assert re.search(r"enum \{ MIRT_DENOISE_SRC_ACCUM = 0, MIRT_DENOISE_SRC_ADAPT = 1 \};", HEADER)
    assert re.search(r"enum \{ MIRT_DENOISE_OUT_F32 = 1u << 0 \};", HEADER)
    for name, text, value in (("MIRT_DENOISE_SRC_ACCUM", "0", 0), ("MIRT_DENOISE_SRC_ADAPT", "1", 1), ("MIRT_DENOISE_OUT_F32", "1 << 0", 1)):
        assert re.search(r"pub const %s: u32 = %s;" % (name, re.escape(text)), RS), name
        assert getattr(_abi, name) == value == getattr(m, name)
    assert dr.TONE_FLAGS == _abi.MIRT_FLAG_NO_TONEMAP | _abi.MIRT_FLAG_NO_SRGB and dr.MISS == _abi.MIRT_RAY_MISS
    assert dr.FEATURE_DTYPE == FEATURE_DTYPE
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0          # a new capability, no new version, no new status code
    assert "MIRT_ERR_DENOISE" not in HEADER


def test_a_null_pointer_is_refused_before_any_device_call():
    lib = m.lib()
    p = m.make_params(4, 2, 0)
    good = m.make_denoise_params("accum")
    bad = m.make_denoise_params("adapt", levels=99, sigma_colour=-1.0)
    guides = np.zeros(8, FEATURE_DTYPE)
    out = np.full(8 * 16, 0xA5, np.uint8)
    pg, po = C.c_void_p(guides.ctypes.data), C.c_void_p(out.ctypes.data)
    for d in (good, bad, None):
        for params, g, o in ((C.byref(p), pg, po), (None, pg, po), (C.byref(p), None, po), (C.byref(p), pg, None)):
            dd = C.byref(d) if d is not None else None
            assert lib.mirt_ctx_denoise(None, params, dd, g, guides.nbytes, o, out.nbytes) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_denoise_device(None, params, dd, g, guides.nbytes, o, out.nbytes, None) == _abi.MIRT_ERR_NULL_POINTER
    assert b"ctx" in lib.mirt_last_error()
    assert (out == 0xA5).all()


# ---- the Python wrappers' argument checks, against a context that does not exist ----

class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


def test_make_denoise_params_fills_the_struct():
    d = m.make_denoise_params("adapt", levels=5, sigma_colour=0.25, normal_log2=7, f32=True)
    assert (d.source, d.levels, d.normal_log2, d.flags, d.sigma_colour) == (1, 5, 7, 1, 0.25) and list(d._pad) == [0, 0, 0]
    d = m.make_denoise_params()
    assert (d.source, d.levels, d.normal_log2, d.flags, d.sigma_colour) == (0, 3, 5, 0, 1.0)


@pytest.mark.parametrize("kw", [dict(source="sums"), dict(source=0), dict(source=None), dict(levels=3.0), dict(levels=True), dict(levels=-1), dict(levels="3"),
                                dict(normal_log2=2 ** 32), dict(normal_log2=None), dict(sigma_colour="1"), dict(sigma_colour=None), dict(sigma_colour=True),
                                dict(f32=1), dict(f32=None)], ids=str)
def test_make_denoise_params_refuses_wrong_types(kw):
    source = kw.pop("source", "accum")
    with pytest.raises(ValueError):
        m.make_denoise_params(source, **kw)


@pytest.mark.parametrize("params", [None, (67, 45, 0), {"width": 67}, "params"], ids=["None", "tuple", "dict", "str"])
def test_the_wrappers_refuse_params_that_are_no_params(params, no_library):
    d, g = m.make_denoise_params(), np.zeros((2, 4), FEATURE_DTYPE)
    with pytest.raises(ValueError):
        Context.denoise(_NoLibrary(), params, d, g)
    with pytest.raises(ValueError):
        Context.denoise_device(_NoLibrary(), params, d, 0x1000, 256, 0x2000, 32)


@pytest.mark.parametrize("denoise", [None, 3, {"levels": 3}, "accum", _abi.MirtAdaptParams()], ids=["None", "int", "dict", "str", "another struct"])
def test_the_wrappers_refuse_a_denoise_that_is_no_struct(denoise, no_library):
    p, g = m.make_params(4, 2, 0), np.zeros((2, 4), FEATURE_DTYPE)
    with pytest.raises(ValueError):
        Context.denoise(_NoLibrary(), p, denoise, g)
    with pytest.raises(ValueError):
        Context.denoise_device(_NoLibrary(), p, denoise, 0x1000, 256, 0x2000, 32)


@pytest.mark.parametrize("guides", [None, np.zeros((2, 4, 8), np.float32), np.zeros(8, np.uint8), [1, 2], "guides"], ids=["None", "float32", "bytes", "list", "str"])
def test_denoise_refuses_guides_that_are_no_feature_records(guides, no_library):
    with pytest.raises(ValueError):
        Context.denoise(_NoLibrary(), m.make_params(4, 2, 0), m.make_denoise_params(), guides)


@pytest.mark.parametrize("args", [(0, 256, 0x2000, 32), (-8, 256, 0x2000, 32), (None, 256, 0x2000, 32), (1.0, 256, 0x2000, 32), (True, 256, 0x2000, 32),
                                  (0x1000, -1, 0x2000, 32), (0x1000, 1.5, 0x2000, 32), (0x1000, None, 0x2000, 32), (0x1000, True, 0x2000, 32),
                                  (0x1000, 256, 0, 32), (0x1000, 256, None, 32), (0x1000, 256, 2.0, 32), (0x1000, 256, 0x2000, -1), (0x1000, 256, 0x2000, None),
                                  (0x1000, 256, 0x2000, 0.5)], ids=str)
def test_denoise_device_refuses_pointers_that_are_no_addresses_and_sizes_that_are_no_counts(args, no_library):
    with pytest.raises(ValueError):
        Context.denoise_device(_NoLibrary(), m.make_params(4, 2, 0), m.make_denoise_params(), *args)


# ---- the rule on the CPU ----

def test_the_level_scales_and_what_the_library_accepts():
    assert [float(v) for v in dr.level_scales(1.0, 4)] == [1.0, 4.0, 16.0, 64.0]
    assert [float(v) for v in dr.level_scales(0.5, 2)] == [4.0, 16.0] and dr.level_scales(0.0, 3) == [None] * 3
    for sigma, levels, ok in ((0.0, 8, True), (-0.0, 3, True), (1.0, 8, True), (-1.0, 1, False), (float("nan"), 1, False), (float("inf"), 1, False),
                              (1e-30, 1, False), (1e30, 1, False), (1e-18, 3, True), (1e18, 3, True), (5e-18, 3, True), (5e-18, 8, False), (2e-17, 8, True)):
        assert dr.scales_valid(sigma, levels) == ok, (sigma, levels)


def _small_frame():
    rng = np.random.default_rng(1)
    R, W = 7, 9
    g = np.zeros((R, W), FEATURE_DTYPE)
    g["albedo"] = rng.uniform(0, 1, (R, W, 3)).astype(f32)
    n = rng.normal(size=(R, W, 3))
    g["normal"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(f32)
    g["sphere"] = rng.integers(0, 3, (R, W))
    g["sphere"][0, :4] = dr.MISS
    g["sphere"][5, 3:] = dr.MISS
    g["albedo"][1, 1] = [np.nan, np.inf, -1]
    g["albedo"][4, 4] = [1e-9, 1e9, 64]
    g["albedo"][0, 1] = [np.nan, np.nan, np.nan]                     # on a miss: not read
    g["normal"][2, 2] = [np.nan, 1, 0]
    g["normal"][3, 3] = [np.inf, 0, 0]
    g["normal"][3, 4] = [-np.inf, np.inf, np.nan]
    g["normal"][6, 6] = [3e38, 3e38, 3e38]
    sums = rng.integers(0, 4 << 20, (R, W, 3)).astype(np.uint64) * np.uint64(5)
    sums[2, 5] = 2 ** 64 - 1
    cnt = rng.integers(0, 9, (R, W)).astype(np.uint32)
    cnt[2, 5] = 1
    return sums, cnt, g


@pytest.mark.parametrize("sigma, nl", [(1.0, 5), (0.0, 5), (0.25, 0), (1.0, 8)])
def test_the_two_restatements_agree_bit_for_bit(sigma, nl):
    sums, cnt, g = _small_frame()
    assert (cnt == 0).any() and np.isnan(g["normal"]).any() and np.isinf(g["albedo"]).any()
    for flags in (0, dr.TONE_FLAGS):
        a, b = dr.denoise(sums, cnt, g, 3, sigma, nl, flags), dr.denoise_naive(sums, cnt, g, 3, sigma, nl, flags)
        assert np.isfinite(a[0]).all() and (a[0][..., 3] == 1).all() and (a[1][..., 3] == 255).all()
        assert dr.same_f32(a[0], b[0]) and np.array_equal(a[1], b[1])
    raw = dr.means(sums, cnt)
    assert not np.array_equal(a[0][..., :3], raw)                       # the filter does something


def test_the_rgba8_form_is_the_resolve_of_the_linear_form():
    sums, cnt, g = _small_frame()
    lin, rgba = dr.denoise(sums, cnt, g, 2, 1.0, 5)
    assert np.array_equal(rgba[..., :3], ob.resolve_channel(ob.to_fixed(lin[..., :3]).astype(np.uint64), 1, 0))
    # one level, no colour weight, every pixel its own sphere: the frame is the means themselves (36 c / 36, then c x den)
    g2 = g.copy()
    g2["sphere"] = np.arange(g.size).reshape(g.shape)
    den = dr.divisors(g2)
    c = (dr.means(sums, cnt) / den).astype(f32)
    want = ((((f32(36.0) * c).astype(f32) / f32(36.0)).astype(f32)) * den).astype(f32)
    assert dr.same_f32(dr.denoise(sums, cnt, g2, 1, 0.0, 5)[0][..., :3], want)


# ---- the quality condition, on the CPU reference alone ----

QW, QH = 192, 128


@functools.lru_cache(maxsize=None)
def _three_spheres():
    scene, cam = m.scenes.three_spheres()
    mats, tex = m.flatten_materials(scene.materials)
    gc = m.GpuCamera.new(cam, (QW, QH))
    cs = [s.to_c() for s in scene.spheres]
    sd = m.SceneData(gc.c, cs, list(mats), tex, None)
    arr = hbm_worlds.sphere_array([list(s.center[:3]) for s in cs], [s.radius for s in cs], [s.material_idx for s in cs])
    ref = fr.FeatureRef(arr, mats, tex, gc.c, QW, QH)
    truth = dr.means(ob.render_pt_sums(sd, m.make_params(QW, QH, 2048, mode=m.MIRT_MODE_PT, num_bounces=8, sample_begin=4096)), 2048)
    return sd, ref, truth


@pytest.mark.parametrize("spp", [4, 16])
def test_the_filtered_frame_is_closer_to_the_truth_than_the_raw_one(spp):
    """Measured: raw 0.002546 -> filtered 0.00130 at 4 spp, raw 0.000653 -> filtered 0.00048 at 16 spp."""
    sd, ref, truth = _three_spheres()
    sums = ob.render_pt_sums(sd, m.make_params(QW, QH, spp, mode=m.MIRT_MODE_PT, num_bounces=8))
    guides = ref.frame(spp)
    raw = dr.mse(dr.means(sums, spp), truth)
    filtered = dr.mse(dr.denoise(sums, spp, guides, 3, 1.0, 5)[0], truth)
    print(f"three_spheres {QW} x {QH}, {spp} spp: raw MSE {raw:.6f}, filtered MSE {filtered:.6f}")
    assert filtered < raw
