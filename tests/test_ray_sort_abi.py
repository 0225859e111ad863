"""MIRT_RAYS_SORT / MIRT_RADIANCE_SORT through the layers that need no device: exports, arities and constants across the header, the
ctypes mirror, the C++ mirror and the Rust crate's source; mirt_ray_sort_code against the numpy restatement of the header's text
(tests/ray_sort_ref.py) on camera rays, degenerate rays and degenerate bounds; the audit of the two ray sets the device tests order
(D: all codes distinct, T: all codes equal); null pointers and the wrappers' argument checks."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, RADIANCE_RAY_DTYPE, RAY_DTYPE, RAY_HIT_DTYPE
import feature_ref as fr
import ray_query_ref as rq
import ray_sort_ref as rs

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
NEW = {"mirt_ray_sort_code": 4, "mirt_ctx_trace_order_read": 3}
f32 = np.float32


def test_the_library_exports_the_two_symbols():
    lib = m.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.SYMBOLS, name


def test_header_ctypes_cpp_and_rust_agree_on_arity():
    for name, arity in NEW.items():
        h = re.search(r"^int %s\s*\(([^)]*)\)\s*;" % name, HEADER, re.M)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, RS)
        assert h and r, name
        count = lambda args: len([a for a in args.split(",") if a.strip()])
        assert count(h.group(1)) == count(r.group(1)) == len(_abi.SYMBOLS[name][1]) == arity, name
        assert _abi.SYMBOLS[name][0] is C.c_int
        call = re.search(r"check\(%s\(([^;]*)\)\);" % name, HPP)             # the C++ mirror calls it with as many arguments
        assert call and count(call.group(1)) == arity, name


def test_constants_match_the_header_and_the_crate():
    for family, old in (("RAYS", ("FLAT", "ANY_HIT", "COUNT")), ("RADIANCE", ("FLAT", "ACCUMULATE", "SKY_HOSEK"))):
        enum = re.search(r"enum \{ (MIRT_%s_FLAT[^}]*)\}" % family, HEADER).group(1)
        names = dict((n, int(s)) for n, s in re.findall(r"(MIRT_\w+) = 1u << (\d+)", enum))
        want = {"MIRT_%s_%s" % (family, o): k for k, o in enumerate(old)}
        want["MIRT_%s_SORT" % family] = 4
        assert names == want, names                                          # bit 3 is assigned to nothing
        for name, shift in want.items():
            assert re.search(r"pub const %s: u32 = 1 << %d;" % (name, shift), RS), name
            assert getattr(_abi, name) == 1 << shift == getattr(m, name)
        assert not re.search(r"pub const MIRT_%s_\w+: u32 = 1 << 3;" % family, RS)
        assert not any(getattr(_abi, n) == 8 for n in dir(_abi) if n.startswith("MIRT_%s_" % family))
    for name, value in (("MIRT_RAY_SORT_ORIGIN_BITS", 5), ("MIRT_RAY_SORT_DIRECTION_BITS", 8)):
        assert re.search(r"#define %s\s+%du\b" % (name, value), HEADER), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), RS), name
        assert getattr(_abi, name) == value == getattr(m, name)
    assert (rs.ORIGIN_BITS, rs.DIRECTION_BITS) == (5, 8) and 3 * rs.ORIGIN_BITS + 2 * rs.DIRECTION_BITS == 31
    assert re.search(r'#include "[./]*include/mirt.h"', HPP)                  # the C++ mirror takes the constants from the header
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0                # a new capability, no new version


# ---- mirt_ray_sort_code against the header's text ----

def _lib_codes(centre, radius, o, d, dtype=RAY_DTYPE):
    rays = np.zeros(len(o), dtype)
    rays["origin"], rays["direction"] = o, d
    if dtype == RAY_DTYPE:
        rays["t_max"], rays["_pad"] = 1000.0, np.nan                         # neither is read
    else:
        rays["stream"], rays["_pad"] = np.arange(len(o)), 0xFFFFFFFF
    return m.ray_sort_codes(centre, radius, rays)


def _same(centre, radius, o, d, what):
    got, want = _lib_codes(centre, radius, o, d), rs.codes(centre, radius, o, d)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(o)} codes differ, first ray {bad[0]}: o {o[bad[0]]} d {d[bad[0]]} -> {got[bad[0]]:#x}, want {want[bad[0]]:#x}"
    assert (got >> 31 == 0).all()
    return got


@pytest.fixture(scope="module")
def bounds():
    return rs.world_bounds(fr.fixture().arr)


def test_the_code_of_camera_rays(bounds):
    ys, xs = np.divmod(np.arange(rs.N), fr.W)
    o, d = fr.centre_rays(fr.fixture_camera(), fr.W, fr.H, xs, ys)
    code = _same(*bounds, o, d, "centre rays")
    assert len(np.unique(code >> 16)) == 1 and len(np.unique(code)) > 100    # one origin cell; the direction bits order them
    # MirtRadianceRay records give the same codes: the layout the function reads is shared
    assert np.array_equal(_lib_codes(*bounds, o, d, RADIANCE_RAY_DTYPE), code)
    o, d = fr.sample_rays(fr.fixture_camera(0.1), fr.W, fr.H, xs, ys, 0, 0)
    code = _same(*bounds, o, d, "lens rays")
    assert len(np.unique(o, axis=0)) > 3000                                  # an origin per ray
    # probes: origins all over the bounds (and a little outside: clamped), a sphere of directions each -- every origin bit and both
    # halves of the octahedron in use
    rng = np.random.default_rng(9)
    o, d = rng.uniform(-1.1, 1.1, (4096, 3)).astype(f32), rng.normal(size=(4096, 3)).astype(f32)
    code = _same(np.zeros(3, f32), 1.0, o, d, "probe rays")
    m3, m2 = code >> 16, code & 0xFFFF
    assert np.bitwise_or.reduce(m3) == 0x7FFF and np.bitwise_or.reduce(m2) == 0xFFFF and (d[:, 2] < 0).sum() > 1000


def test_the_code_of_degenerate_rays_and_bounds(bounds):
    o, d, defined = rq.degenerate_rays()
    assert (~defined).sum() >= 128
    _same(*bounds, o, d, "degenerate rays")
    zero = ~(d != 0).any(1)
    assert (rs.codes(*bounds, o, d)[zero] & 0xFFFF == 0).all()               # 1 / 0 = inf, 0 * inf = NaN, q(NaN) = 0
    far = np.array([[3e38, -3e38, 1e-45], [np.inf, -np.inf, np.nan], [-0.0, 0.0, 5.0]], f32)
    both_o, both_d = np.concatenate([o, far, o[:3]]), np.concatenate([d, d[:3], far])
    centre = bounds[0]
    for radius in (0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, -7.5):
        _same(centre, radius, both_o, both_d, f"radius {radius}")
    for c in ([np.nan, 0, 0], [np.inf, -np.inf, 0], [3e38, -3e38, 0], [0, 0, 0]):
        _same(np.array(c, f32), bounds[1], both_o, both_d, f"centre {c}")
    _same(np.zeros(3, f32), 0.0, both_o, both_d, "the bounds of an empty tree")


def test_set_d_has_3015_distinct_codes_and_set_t_one(bounds):
    o, d = rs.set_d()
    assert rs.D_FOV == 180.0 and len(o) == rs.N == 3015
    code = _same(*bounds, o, d, "D")
    assert len(np.unique(code)) == 3015
    assert len(np.unique(code & 0xFFFF)) == 3015                             # by direction alone: whatever bounds a resident tree reports
    assert len(np.unique(o, axis=0)) == 1
    order = rs.order_of(code)
    assert not np.array_equal(order, np.arange(rs.N))                        # the image order is not the sorted order: a sorted launch shows
    p = rs.permutation(rs.N)
    assert np.array_equal(p[rs.order_of(code[p])], order)                    # the same rays in the same slots, however D is handed over
    for fov, distinct in ((90.0, False), (120.0, True), (270.0, True), (300.0, False)):         # the field of view is chosen, not lucky
        assert (len(np.unique(rs.codes(*bounds, o, rs.d_directions(fov)))) == 3015) == distinct, fov
    o, d = rs.set_t()
    code = _same(*bounds, o, d, "T")
    assert len(o) == 3015 and len(np.unique(code)) == 1
    assert np.array_equal(rs.order_of(code), np.arange(rs.N))


# ---- refusals ----

def test_null_pointers_are_refused():
    lib = m.lib()
    centre, ray, code = (C.c_float * 3)(), (C.c_float * 8)(), C.c_uint32(0xABCD)
    args = [centre, C.c_float(1.0), C.cast(ray, C.c_void_p), C.byref(code)]
    assert lib.mirt_ray_sort_code(*args) == _abi.MIRT_OK and code.value != 0xABCD
    code.value = 0xABCD
    for k in (0, 2, 3):
        a = list(args)
        a[k] = None
        assert lib.mirt_ray_sort_code(*a) == _abi.MIRT_ERR_NULL_POINTER
    assert code.value == 0xABCD
    order = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.mirt_ctx_trace_order_read(None, C.cast(order, C.c_void_p), 4) == _abi.MIRT_ERR_NULL_POINTER
    assert b"ctx" in lib.mirt_last_error() and list(order) == [7, 7, 7, 7]
    # a null context with the new flags: as with every other flag word
    rays, hits = (_abi.MirtRay * 2)(), (_abi.MirtRayHit * 2)()
    for flags in (_abi.MIRT_RAYS_SORT, _abi.MIRT_RAYS_SORT | 7, _abi.MIRT_RAYS_SORT | 8):
        assert lib.mirt_ctx_trace_rays(None, C.cast(rays, C.c_void_p), 2, flags, C.cast(hits, C.c_void_p)) == _abi.MIRT_ERR_NULL_POINTER
        p = _abi.MirtRadianceParams(4, 0, 8, flags, 0)
        assert lib.mirt_ctx_trace_radiance(None, C.cast(rays, C.c_void_p), 2, C.byref(p), C.cast(hits, C.c_void_p)) == _abi.MIRT_ERR_NULL_POINTER
    assert not any(bytes(hits))


class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("sort", [1, 0, None, "yes", _abi.MIRT_RAYS_SORT], ids=repr)
def test_the_wrappers_refuse_a_sort_that_is_no_bool(sort, no_library):
    with pytest.raises(ValueError):
        Context.trace_rays(_NoLibrary(), np.zeros(2, RAY_DTYPE), 0, sort=sort)
    with pytest.raises(ValueError):
        Context.trace_rays_device(_NoLibrary(), 0x1000, 2, 0x2000, 0, sort=sort)
    with pytest.raises(ValueError):
        Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), 4, sort=sort)
    with pytest.raises(ValueError):
        Context.trace_radiance_device(_NoLibrary(), 0x1000, 2, 0x2000, 4, sort=sort)


@pytest.mark.parametrize("flags", [8, 16 | 8, 32, 16 | 32])
def test_the_wrappers_still_refuse_unassigned_bits_beside_the_sort_bit(flags, no_library):
    with pytest.raises(ValueError):
        Context.trace_rays(_NoLibrary(), np.zeros(2, RAY_DTYPE), flags)


@pytest.mark.parametrize("kw", [dict(rays=np.zeros((2, 8), f32)), dict(rays=np.zeros(2, RAY_HIT_DTYPE)), dict(rays=[1]), dict(centre=[0, 0]), dict(centre=np.zeros((3, 1))),
                                dict(radius="1"), dict(radius=None), dict(radius=True)], ids=lambda kw: next(iter(kw)))
def test_ray_sort_codes_refuses_what_is_no_ray_array_or_no_bounds(kw, no_library):
    args = dict(centre=np.zeros(3, f32), radius=1.0, rays=np.zeros(2, RAY_DTYPE))
    args.update(kw)
    with pytest.raises(ValueError):
        m.ray_sort_codes(**args)
