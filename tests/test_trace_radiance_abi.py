"""mirt_ctx_trace_radiance and mirt_ctx_trace_radiance_device through the layers that need no device: the library's exports and its
checks before any HIP call, the ctypes mirror's layout against the header and the Rust crate's source, and the Python wrappers'
argument checks -- and an audit, on the CPU oracle alone, that the ray set of tests/test_gpu_trace_radiance.py exercises what it is
meant to."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, RADIANCE_DTYPE, RADIANCE_RAY_DTYPE, RAY_DTYPE, radiance_ray_records
import radiance_ref as rr
import ray_query_ref as rq

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
NEW = {"mirt_ctx_trace_radiance": 5, "mirt_ctx_trace_radiance_device": 6}
STRUCTS = {"MirtRadianceRay": 32, "MirtRadiance": 32, "MirtRadianceParams": 24}
FLAGS = (("MIRT_RADIANCE_FLAT", 0), ("MIRT_RADIANCE_ACCUMULATE", 1), ("MIRT_RADIANCE_SKY_HOSEK", 2))


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


def test_struct_sizes_offsets_and_field_order():
    R, O, P = _abi.MirtRadianceRay, _abi.MirtRadiance, _abi.MirtRadianceParams
    assert (C.sizeof(R), C.sizeof(O), C.sizeof(P)) == (32, 32, 24)
    assert (R.origin.offset, R.stream.offset, R.direction.offset, R._pad.offset) == (0, 12, 16, 28)
    assert (O.sum.offset, O.samples.offset, O._pad.offset) == (0, 24, 28)
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16]
    # the numpy records the wrappers move are the same bytes
    assert RADIANCE_RAY_DTYPE.itemsize == 32 and [RADIANCE_RAY_DTYPE.fields[f][1] for f in ("origin", "stream", "direction", "_pad")] == [0, 12, 16, 28]
    assert RADIANCE_DTYPE.itemsize == 32 and [RADIANCE_DTYPE.fields[f][1] for f in ("sum", "samples", "_pad")] == [0, 24, 28]
    assert RADIANCE_RAY_DTYPE.fields["stream"][0] == np.dtype("<u4") and RADIANCE_DTYPE.fields["sum"][0].base == np.dtype("<u8")
    # header and Rust source list the fields of the ctypes mirror, in its order
    for name, size in STRUCTS.items():
        py = [f for f, _ in getattr(_abi, name)._fields_]
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), HEADER, re.S).group(1)
        in_header = [w for decl in body.split(";") if decl.strip() for w in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", re.sub(r"^\s*\w+\s+", "", decl.strip()))]
        assert in_header == py, (name, in_header)
        rust = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct %s \{(.*?)\n\}" % name, RS, re.S)
        assert rust and re.findall(r"pub (\w+):", rust.group(1)) == py, name
        assert HEADER.count("sizeof(%s) == %d" % (name, size)) == 2, name            # static_assert and _Static_assert


def test_constants_match_the_header_and_the_crate():
    enum = re.search(r"enum \{ (MIRT_RADIANCE_FLAT[^}]*)\}", HEADER).group(1)
    for name, shift in FLAGS:
        assert re.search(r"%s = 1u << %d\b" % (name, shift), enum), name
        assert re.search(r"pub const %s: u32 = 1 << %d;" % (name, shift), RS), name
        assert getattr(_abi, name) == 1 << shift == getattr(m, name)
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0    # a new capability, no new version


def test_null_context_params_and_pointers_are_refused_before_any_device_call():
    lib = m.lib()
    rays, out = (_abi.MirtRadianceRay * 2)(), (_abi.MirtRadiance * 2)()
    pr, po = C.cast(rays, C.c_void_p), C.cast(out, C.c_void_p)
    before = bytes(out)
    for flags in (0, _abi.MIRT_RADIANCE_FLAT, 7, 8, 0xFFFFFFFF):
        p = _abi.MirtRadianceParams(4, 0, 8, flags, 0)
        for n, a, b in ((2, pr, po), (0, None, None), (2, None, po), (2, pr, None), (0, pr, po)):
            assert lib.mirt_ctx_trace_radiance(None, a, n, C.byref(p), b) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_trace_radiance_device(None, a, n, C.byref(p), b, None) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_trace_radiance(None, a, n, None, b) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_trace_radiance_device(None, a, n, None, b, None) == _abi.MIRT_ERR_NULL_POINTER
    assert b"ctx" in lib.mirt_last_error()
    assert bytes(out) == before                                   # a refused call writes nothing


# ---- the Python wrappers' argument checks, against a context that does not exist ----

class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("bad", [np.zeros((4, 6), np.uint32), np.zeros((4, 8), np.float32), np.zeros((4, 8), np.uint64), np.zeros((2, 2), RADIANCE_RAY_DTYPE),
                                 np.zeros(8, np.uint32), np.zeros(3, RADIANCE_DTYPE), np.zeros(3, RAY_DTYPE), [[0] * 8], "rays", None, 3],
                         ids=["[n, 6]", "f32 [n, 8]", "u64", "2-d records", "1-d words", "output records", "MirtRay records", "list", "str", "None", "int"])
def test_trace_radiance_refuses_a_wrong_dtype_or_shape(bad, no_library):
    with pytest.raises(ValueError):
        Context.trace_radiance(_NoLibrary(), bad, 4)


@pytest.mark.parametrize("into", [np.zeros(3, RADIANCE_DTYPE), np.zeros((2, 1), RADIANCE_DTYPE), np.zeros(2, RADIANCE_RAY_DTYPE), np.zeros(4, RADIANCE_DTYPE)[::2],
                                  np.zeros((2, 4), np.uint64), [0, 0], 0],
                         ids=["too long", "2-d", "ray records", "strided", "u64 [n, 4]", "list", "int"])
def test_trace_radiance_refuses_records_it_cannot_accumulate_into(into, no_library):
    with pytest.raises(ValueError):
        Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), 4, into=into)
    ro = np.zeros(2, RADIANCE_DTYPE)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), 4, into=ro)


@pytest.mark.parametrize("kw", [dict(flat=1), dict(flat=None), dict(hosek=4), dict(hosek="yes"), dict(flat=_abi.MIRT_RADIANCE_FLAT), dict(accumulate=2)],
                         ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_the_wrappers_refuse_flags_that_are_no_bools(kw, no_library):
    if "accumulate" not in kw:
        with pytest.raises(ValueError):
            Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), 4, **kw)
    with pytest.raises(ValueError):
        Context.trace_radiance_device(_NoLibrary(), 0x1000, 2, 0x2000, 4, **kw)


@pytest.mark.parametrize("kw", [dict(spp=-1), dict(spp=1 << 32), dict(spp=1.0), dict(spp=True), dict(spp=None), dict(sample_begin=-1), dict(sample_begin=1 << 32),
                                dict(num_bounces=-1), dict(num_bounces=2.5), dict(num_bounces=1 << 32), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)],
                         ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_the_wrappers_refuse_params_that_do_not_fit_the_struct(kw, no_library):
    spp = kw.pop("spp", 4)
    with pytest.raises(ValueError):
        Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), spp, **kw)
    with pytest.raises(ValueError):
        Context.trace_radiance_device(_NoLibrary(), 0x1000, 2, 0x2000, spp, **kw)


@pytest.mark.parametrize("d_rays, n, d_out", [(0x1000, -1, 0x2000), (0x1000, 2 ** 32, 0x2000), (0x1000, 1.5, 0x2000), (0x1000, True, 0x2000),
                                                (0, 4, 0x2000), (0x1000, 4, 0), (-8, 4, 0x2000), (0x1000, 4, None), (1.0, 4, 0x2000), (True, 4, 0x2000)])
def test_trace_radiance_device_refuses_a_count_that_is_no_u32_and_pointers_that_are_no_addresses(d_rays, n, d_out, no_library):
    with pytest.raises(ValueError):
        Context.trace_radiance_device(_NoLibrary(), d_rays, n, d_out, 4)


def test_make_radiance_rays_and_the_records_keep_the_bits():
    raw = np.arange(24, dtype=np.uint32).reshape(3, 8) * np.uint32(0x01010101) + np.uint32(0x7fc00001)     # NaN payloads among them
    recs = radiance_ray_records(raw)
    assert recs.dtype == RADIANCE_RAY_DTYPE and recs.shape == (3,) and np.array_equal(recs.view(np.uint32).reshape(3, 8), raw)
    assert np.array_equal(recs["stream"], raw[:, 3]) and np.array_equal(recs["origin"].view(np.uint32), raw[:, :3])
    assert radiance_ray_records(recs) is recs or np.shares_memory(radiance_ray_records(recs), recs)
    rays = m.make_radiance_rays((1, 2, 3), [[0, 0, -1], [0, -0.0, 1], [np.nan, np.inf, 1e-45]])
    assert rays.dtype == RADIANCE_RAY_DTYPE and rays["stream"].tolist() == [0, 1, 2]                     # default: the ray's index
    assert rays["origin"].tolist() == [[1, 2, 3]] * 3 and np.signbit(rays["direction"][1, 1]) and not rays["_pad"].any()
    assert np.isnan(rays["direction"][2, 0]) and np.isinf(rays["direction"][2, 1]) and rays["direction"][2, 2] == np.float32(1e-45)
    assert np.array_equal(rays["direction"][0].view(np.uint32), np.array([0, 0, 0xbf800000], np.uint32))  # used as given: not normalised
    assert m.make_radiance_rays(np.zeros((2, 3)), np.ones((2, 3)) * 3, [7, 0xffffffff])["stream"].tolist() == [7, 0xffffffff]
    assert m.make_radiance_rays(np.zeros((2, 3)), np.ones((2, 3)), 5)["stream"].tolist() == [5, 5]
    for bad in ([-1, 0], [0, 1 << 32], [0.5, 1.0]):
        with pytest.raises(ValueError):
            m.make_radiance_rays(np.zeros((2, 3)), np.ones((2, 3)), bad)


def test_radiance_mean_divides_the_exact_sums():
    rec = np.zeros(3, RADIANCE_DTYPE)
    rec["sum"] = [[1 << 20, 2 << 20, 0], [3 << 19, 0, 1], [0, 0, 0]]
    rec["samples"] = [1, 3, 0]
    assert np.array_equal(m.radiance_mean(rec), np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 2.0 ** -20 / 3], [0, 0, 0]]))


# ---- the ray set of the GPU tests is not vacuous: asserted on the oracle and the CPU restatement of the flat scan alone ----

def test_the_ray_set_exercises_every_routine_the_hollow_hero_and_the_sky():
    arr, mats, _ = rr.world()
    o, d, llc = rr.ray_set()
    assert o.shape == d.shape == (rr.N_RAYS, 3) and o.dtype == d.dtype == np.float32 and np.array_equal(d, llc - o)
    hits = rr.first_hits()
    hit = hits["sphere"] != rq.MISS
    ids = {int(mats[int(arr["material_idx"][s])].id) for s in hits["sphere"][hit]}
    assert ids >= {0, 1, 2, 3, 7}, ids                               # lambertian, metal, dielectric, checkerboard and the missing-material id
    mat_idx = set(arr["material_idx"][hits["sphere"][hit]].tolist())
    assert {0, 1} <= mat_idx                                         # a colour texture and the image texture
    assert hits["sphere"][rr.MISSES_ALL] == rq.MISS and (~hit).sum() >= 2
    # one ray starts inside the hollow glass hero: inside its outer sphere (index 1, r = 1) AND its inner one (index 2, r = -0.9)
    c = arr["center"][1, :3].astype(np.float64)
    assert arr["radius"][1] == 1.0 and arr["radius"][2] == np.float32(-0.9) and np.array_equal(arr["center"][1], arr["center"][2])
    assert np.linalg.norm(o[rr.INSIDE_HERO] - c) < 0.9 and hits["sphere"][rr.INSIDE_HERO] == 2
    assert len(np.unique(hits["sphere"][hit])) >= 10                 # measured: 13 distinct first spheres


def test_the_oracles_sums_differ_between_streams_and_follow_every_parameter():
    sums = np.stack([rr.oracle_sums(i) for i in range(rr.N_RAYS)])                                   # [32, 8, 3]
    assert sums.shape == (rr.N_RAYS, rr.N_STREAMS, 3) and sums.dtype == np.uint64
    differ = [(sums[i] != sums[i][0]).any() for i in range(rr.N_RAYS)]
    distinct = [len({tuple(r) for r in sums[i].tolist()}) for i in range(rr.N_RAYS)]
    assert sum(differ) >= 24 and sum(n == rr.N_STREAMS for n in distinct) >= 20, distinct              # measured: 28 rays, all with 8 different sums
    assert not differ[rr.MISSES_ALL] and sums[rr.MISSES_ALL].all()                                    # the sky alone: no draw decides anything
    assert sums.any(2).all(1).sum() >= 24                            # most rays bring light back within 8 bounces
    for kw in (dict(sample_begin=5), dict(seed=rr.SEED), dict(hosek=True), dict(num_bounces=1), dict(spp=5)):
        assert not np.array_equal(rr.oracle_sums(1, **kw), rr.oracle_sums(1)), kw
    # paths longer than 8 segments exist among the rays the bounce test takes: 300 bounces change their sums
    assert sum(not np.array_equal(rr.oracle_sums(i, num_bounces=300), rr.oracle_sums(i)) for i in rr.BOUNCE_RAYS) >= 2
    assert not np.stack([rr.oracle_sums(i, num_bounces=0) for i in range(rr.N_RAYS)]).any()
    with pytest.raises(ValueError):
        rr.oracle_sums(0)[0, 0] = 1                                  # shared between tests: read-only


def test_the_probe_camera_is_accepted_as_a_pinhole_camera_by_the_oracle_only_through_its_rays():
    """Two different probe cameras for the same ray bits give the same sums: nothing but (eye, llc - eye) reaches the paths."""
    o, d, llc = rr.ray_set()
    arr, mats, tex = rr.world()
    p = m.make_params(rr.N_STREAMS, 1, 4, mode=m.MIRT_MODE_PT, num_bounces=8)
    import hbm_worlds, oracle_binding as ob
    for i in (1, 30):
        cam = rr.probe_camera(o[i], llc[i])
        cam._padding5 = 123.0
        cam.lens_radius = 0.0
        wide = ob.render_pt_sums(hbm_worlds.scene_from_arrays(cam, arr, mats, tex), m.make_params(rr.N_STREAMS, 3, 4, mode=m.MIRT_MODE_PT, num_bounces=8), n_threads=1)
        assert np.array_equal(wide[0], rr.oracle_sums(i))            # row 0 of a taller image: the same pixel indices, the same sums
        assert not np.array_equal(wide[1], wide[0])                  # row 1: other pixel indices, other streams, the same ray
