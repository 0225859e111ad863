"""mirt_ctx_trace_rays, mirt_ctx_trace_rays_device and mirt_ctx_trace_stats through the layers that need no device: the library's
exports and its checks before any HIP call, the ctypes mirror's layout, the Rust crate's source, the Python wrappers' argument checks
-- and an audit, on the CPU reference alone, that the ray sets of tests/test_gpu_trace_rays.py exercise what they are named for."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, RAY_DTYPE, RAY_HIT_DTYPE, ray_records
import ray_query_ref as rq

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
NEW = {"mirt_ctx_trace_rays": 5, "mirt_ctx_trace_rays_device": 6, "mirt_ctx_trace_stats": 2}


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


def test_struct_sizes_offsets_and_field_order():
    R, H, S = _abi.MirtRay, _abi.MirtRayHit, _abi.MirtRayStats
    assert (C.sizeof(R), C.sizeof(H), C.sizeof(S)) == (32, 32, 56)
    assert (R.origin.offset, R.t_max.offset, R.direction.offset, R._pad.offset) == (0, 12, 16, 28)
    assert (H.t.offset, H.sphere.offset, H.point.offset, H.normal.offset) == (0, 4, 8, 20)
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48]
    # the numpy records the wrappers move are the same bytes
    assert RAY_DTYPE.itemsize == 32 and [RAY_DTYPE.fields[f][1] for f in ("origin", "t_max", "direction", "_pad")] == [0, 12, 16, 28]
    assert RAY_HIT_DTYPE.itemsize == 32 and [RAY_HIT_DTYPE.fields[f][1] for f in ("t", "sphere", "point", "normal")] == [0, 4, 8, 20]
    # header and Rust source list the fields of the ctypes mirror, in its order
    for name in ("MirtRay", "MirtRayHit", "MirtRayStats"):
        py = [f for f, _ in getattr(_abi, name)._fields_]
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), HEADER, re.S).group(1)
        in_header = [w for decl in body.split(";") if decl.strip() for w in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", re.sub(r"^\s*\w+\s+", "", decl.strip()))]
        assert in_header == py, (name, in_header)
        rust = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct %s \{(.*?)\n\}" % name, RS, re.S)
        assert rust and re.findall(r"pub (\w+):", rust.group(1)) == py, name
    for name in ("sizeof(MirtRay) == 32", "sizeof(MirtRayHit) == 32", "sizeof(MirtRayStats) == 56"):
        assert HEADER.count(name) == 2, name                      # static_assert and _Static_assert


def test_constants_match_the_header_and_the_crate():
    assert re.search(r"#define MIRT_RAY_MISS 0xffffffffu", HEADER) and _abi.MIRT_RAY_MISS == 0xFFFFFFFF == m.MIRT_RAY_MISS
    assert re.search(r"pub const MIRT_RAY_MISS: u32 = 0xffff_ffff;", RS)
    enum = re.search(r"enum \{ (MIRT_RAYS_FLAT[^}]*)\}", HEADER).group(1)
    for name, shift in (("MIRT_RAYS_FLAT", 0), ("MIRT_RAYS_ANY_HIT", 1), ("MIRT_RAYS_COUNT", 2)):
        assert re.search(r"%s = 1u << %d\b" % (name, shift), enum), name
        assert re.search(r"pub const %s: u32 = 1 << %d;" % (name, shift), RS), name
        assert getattr(_abi, name) == 1 << shift == getattr(m, name)
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0    # a new capability, no new version


def test_a_null_context_is_refused_before_any_device_call():
    lib = m.lib()
    rays, hits, stats = (_abi.MirtRay * 2)(), (_abi.MirtRayHit * 2)(), _abi.MirtRayStats()
    pr, ph = C.cast(rays, C.c_void_p), C.cast(hits, C.c_void_p)
    for flags in (0, _abi.MIRT_RAYS_FLAT, 7, 8, 0xFFFFFFFF):
        for n, a, b in ((2, pr, ph), (0, None, None), (2, None, ph), (2, pr, None), (0, pr, ph)):
            assert lib.mirt_ctx_trace_rays(None, a, n, flags, b) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_trace_rays_device(None, a, n, flags, b, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_trace_stats(None, C.byref(stats)) == _abi.MIRT_ERR_NULL_POINTER
    assert b"ctx" in lib.mirt_last_error()


# ---- the Python wrappers' argument checks, against a context that does not exist ----

class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("bad", [np.zeros((4, 6), np.float32), np.zeros((4, 8), np.float64), np.zeros((2, 2), RAY_DTYPE), np.zeros(8, np.float32),
                                 np.zeros(3, RAY_HIT_DTYPE), [[0.0] * 8], "rays", None, 3],
                         ids=["[n, 6]", "f64", "2-d records", "1-d floats", "hit records", "list", "str", "None", "int"])
def test_trace_rays_refuses_a_wrong_dtype_or_shape(bad, no_library):
    with pytest.raises(ValueError):
        Context.trace_rays(_NoLibrary(), bad)


@pytest.mark.parametrize("flags", [8, -1, 1.0, "1", True, None, 1 << 32])
def test_the_wrappers_refuse_flags_that_are_no_rays_flags(flags, no_library):
    with pytest.raises(ValueError):
        Context.trace_rays(_NoLibrary(), np.zeros(2, RAY_DTYPE), flags)
    with pytest.raises(ValueError):
        Context.trace_rays_device(_NoLibrary(), 0x1000, 2, 0x2000, flags)


@pytest.mark.parametrize("d_rays, n, d_hits", [(0x1000, -1, 0x2000), (0x1000, 2 ** 32, 0x2000), (0x1000, 1.5, 0x2000), (0x1000, True, 0x2000),
                                                 (0, 4, 0x2000), (0x1000, 4, 0), (-8, 4, 0x2000), (0x1000, 4, None), (1.0, 4, 0x2000), (True, 4, 0x2000)])
def test_trace_rays_device_refuses_a_count_that_is_no_u32_and_pointers_that_are_no_addresses(d_rays, n, d_hits, no_library):
    with pytest.raises(ValueError):
        Context.trace_rays_device(_NoLibrary(), d_rays, n, d_hits)


def test_ray_records_and_make_rays_keep_the_bits():
    raw = np.arange(24, dtype=np.uint32).reshape(3, 8) * np.uint32(0x01010101) + np.uint32(0x7fc00001)     # NaN payloads among them
    recs = ray_records(raw.view(np.float32))
    assert recs.dtype == RAY_DTYPE and recs.shape == (3,) and np.array_equal(recs.view(np.uint32).reshape(3, 8), raw)
    assert ray_records(recs) is recs or np.shares_memory(ray_records(recs), recs)
    rays = m.make_rays((1, 2, 3), [[0, 0, -1], [0, -0.0, 1]])
    assert rays["t_max"].tolist() == [1000.0, 1000.0] and rays["origin"].tolist() == [[1, 2, 3]] * 2 and np.signbit(rays["direction"][1, 1])
    assert m.make_rays(np.zeros((2, 3)), np.ones((2, 3)), [1.0, np.inf])["t_max"].tolist() == [1.0, np.inf]


def test_pixel_ray_is_the_pinhole_ray_through_the_pixel_centre():
    from grid_rounding import camera_rays
    cam = m.GpuCamera.new(m.FlyCameraController.default().renderer_camera(), (96, 64)).c
    for x, y in ((0, 0), (95, 63), (40, 17)):
        o, d = m.pixel_ray(cam, 96, 64, x, y)
        ro, rd = camera_rays(cam, 96, 64, np.array([(x + 0.5) / 96], np.float32), np.array([(y + 0.5) / 64], np.float32))
        assert np.array_equal(o, ro[0]) and np.allclose(d, rd[0], rtol=0, atol=4e-7 * np.abs(rd[0]).max())
    for x, y in ((-1, 0), (96, 0), (0, 64)):
        with pytest.raises(ValueError):
            m.pixel_ray(cam, 96, 64, x, y)


# ---- the ray sets are not vacuous: asserted on the CPU reference alone ----

def _beside(o, d, c):
    """fp64 distance of centres c from the lines o + t d."""
    O, D, oc = o.astype(np.float64), d.astype(np.float64), o.astype(np.float64) - c.astype(np.float64)
    return np.sqrt(np.maximum((oc * oc).sum(1) - (oc * D).sum(1) ** 2 / (D * D).sum(1), 0.0))


def test_set_a_hits_many_spheres_small_ones_among_them():
    arr, o, d = rq.set_a()
    ref = rq.set_reference("A")
    hit = ref["sphere"] != rq.MISS
    assert len(o) == 4096 and len(arr) == 3000
    # measured: 83.2 % hits, 667 distinct winners, 18.6 % of the rays won by a small sphere (index >= 5)
    assert hit.mean() >= 0.70
    assert len(np.unique(ref["sphere"][hit])) >= 400
    assert (hit & (ref["sphere"] >= 5)).mean() >= 0.10
    assert np.isfinite(ref["normal"][hit]).all() and (ref["t"][hit] > 0.001).all() and (ref["t"][hit] < 1000).all()


def test_set_b_is_decided_by_rounding():
    arr, o, d = rq.set_b()
    ref = rq.set_reference("B")
    cen, rad = rq.world_arrays(arr)
    hit = np.nonzero(ref["sphere"] != rq.MISS)[0]
    w = ref["sphere"][hit]
    # measured: 24.1 % hits; 941 hits whose ray passes more than 10 radii (0.01) beside the winner; 127 zero-radius winners
    assert (_beside(o[hit], d[hit], cen[w]) > 10 * 1e-3).sum() >= 500
    assert (rad[w] == 0).sum() >= 50
    assert len(o) == 4096 and np.isfinite(d).all()
    assert np.isinf(ref["normal"][hit][rad[w] == 0]).any()              # 1 / r = inf reaches the record


def test_set_c_runs_along_the_axes_and_between_the_spheres():
    arr, o, d = rq.set_c()
    ref = rq.set_reference("C")
    hit = ref["sphere"] != rq.MISS
    assert len(o) == 2187 and ((d == 0).sum(1) == 2).all()
    assert 0.15 <= hit.mean() <= 0.35                                   # measured: 23.2 %, 469 distinct winners
    assert len(np.unique(ref["sphere"][hit])) >= 300
    assert ((o * 2) % 2 == 1).any(1).mean() > 0.5                       # origins on half-integer coordinates: between the spheres


def test_the_reference_breaks_ties_to_the_lower_index_and_is_strict_in_t_max():
    cen = np.array([[0, 0, -3]] * 4, np.float32)
    rad = np.full(4, 0.7, np.float32)
    o, d = np.zeros((1, 3), np.float32), np.array([[0, 0, -1]], np.float32)
    ref = rq.trace_ref(o, d, 1000.0, cen, rad)
    assert ref["sphere"][0] == 0 and abs(float(ref["t"][0]) - 2.3) < 1e-6           # the geometric root, rounded as test_sphere rounds it
    t = ref["t"][0]
    assert rq.trace_ref(o, d, t, cen, rad)["sphere"][0] == rq.MISS                                    # t itself: that sphere does not win
    assert rq.trace_ref(o, d, np.nextafter(t, np.float32(np.inf)), cen, rad)["sphere"][0] == 0
    for bound in (np.nan, 0.0, -1.0):
        assert rq.trace_ref(o, d, bound, cen, rad)["sphere"][0] == rq.MISS
    assert rq.trace_ref(o, d, np.inf, cen, rad)["sphere"][0] == 0
    assert rq.same_bits(rq.any_hit_of(ref), np.array([(0, 0, (0, 0, 0), (0, 0, 0))], RAY_HIT_DTYPE)).all()
