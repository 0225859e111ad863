"""mirt_ctx_adapt_* through the layers that need no device: exports, arities, struct layouts and the floor across the header, the ctypes
mirror, the C++ mirror and the Rust crate's source; every error path that needs no device; mirt_adapt_active against the rule in
Python's unlimited integers (tests/adaptive_ref.py) on seeded records and at the rule's corners; and the replay's own footing: one-sample
oracle frames add up to the oracle's render of as many samples."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE, Context
import adaptive_ref as ar
import oracle_binding as ob

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
NEW = {"mirt_adapt_active": 3, "mirt_ctx_adapt_reset": 2, "mirt_ctx_adapt_step_device": 4, "mirt_ctx_adapt_resolve_device": 5,
       "mirt_ctx_adapt_resolve": 4, "mirt_ctx_adapt_read": 3, "mirt_ctx_adapt_write": 3, "mirt_ctx_adapt_list_read": 4, "mirt_ctx_adapt_stats": 2}
STRUCTS = {"MirtAdaptPixel": 64, "MirtAdaptParams": 16, "MirtAdaptStats": 32}


def test_the_library_exports_the_symbols():
    lib = m.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.SYMBOLS, name


def test_header_ctypes_cpp_and_rust_agree_on_arity():
    count = lambda args: len([a for a in args.split(",") if a.strip()])
    for name, arity in NEW.items():
        h = re.search(r"^int %s\s*\(([^)]*)\)\s*;" % name, HEADER, re.M)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, RS)
        assert h and r, name
        assert count(h.group(1)) == count(r.group(1)) == len(_abi.SYMBOLS[name][1]) == arity, name
        assert _abi.SYMBOLS[name][0] is C.c_int
        call = re.search(r"check\(%s\(([^;]*)\)\);" % name, HPP)             # the C++ mirror calls it with as many arguments
        assert call and count(call.group(1)) == arity, name


def test_struct_layouts_and_the_floor():
    P, A, S = _abi.MirtAdaptPixel, _abi.MirtAdaptParams, _abi.MirtAdaptStats
    assert (C.sizeof(P), C.sizeof(A), C.sizeof(S)) == (64, 16, 32)
    assert (P.sum.offset, P.even.offset, P.samples.offset, P._pad0.offset, P._pad1.offset) == (0, 24, 48, 52, 56)
    assert (A.min_samples.offset, A.max_samples.offset, A.tolerance.offset, A.flags.offset) == (0, 4, 8, 12)
    assert (S.pixels.offset, S.total_samples.offset, S.active.offset, S.steps.offset, S.kernel_ms.offset) == (0, 8, 16, 20, 24)
    assert ADAPT_PIXEL_DTYPE.itemsize == 64 and [ADAPT_PIXEL_DTYPE.fields[k][1] for k in ("sum", "even", "samples", "_pad0", "_pad1")] == [0, 24, 48, 52, 56]
    for name, size in STRUCTS.items():
        assert re.search(r"static_assert\(sizeof\(%s\) == %d," % (name, size), HEADER), name
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, RS, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == [f[0] for f in getattr(_abi, name)._fields_], name
    assert re.search(r"typedef struct MirtAdaptPixel \{ uint64_t sum\[3\]; uint64_t even\[3\]; uint32_t samples; uint32_t _pad0; uint64_t _pad1; \}", HEADER)
    assert re.search(r"typedef struct MirtAdaptParams \{ uint32_t min_samples, max_samples, tolerance, flags; \}", HEADER)
    assert re.search(r"#define MIRT_ADAPT_FLOOR \(1u << 17\)", HEADER)
    assert re.search(r"pub const MIRT_ADAPT_FLOOR: u32 = 1 << 17;", RS)
    assert _abi.MIRT_ADAPT_FLOOR == 1 << 17 == m.MIRT_ADAPT_FLOOR == ar.FLOOR
    assert re.search(r"MIRT_ADAPT_FLOOR == 1u << 17", HPP)
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0                # a new capability, no new version


# ---- the rule: mirt_adapt_active against Python's integers ----

def _agree(recs, case, what):
    got = m.adapt_active(recs, m.make_adapt_params(*case))
    want = np.array([ar.record_active(r, *case) for r in recs])
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}, (min, max, tolerance) = {case}: record {bad[0]} {recs[bad[0]]}: library {got[bad[0]]}, rule {want[bad[0]]}"
    return got


def test_the_rule_at_its_corners():
    recs, cases = ar.corner_records()
    assert len(recs) == 128
    seen = set()
    for case in cases:
        got = _agree(recs, case, "corner records")
        seen.update(got.tolist())
    assert seen == {True, False}
    # n = 0 and 1 are active below max_samples whatever the sums say (no halves to compare), and nothing is active at max_samples
    zero = np.zeros(3, ADAPT_PIXEL_DTYPE)
    zero["samples"] = (0, 1, 2)
    assert m.adapt_active(zero, m.make_adapt_params(0, 32, 0xFFFFFFFF)).tolist() == [True, True, False]
    assert m.adapt_active(zero, m.make_adapt_params(0, 2, 0)).tolist() == [True, True, False]
    assert not m.adapt_active(zero, m.make_adapt_params(4, 0, 0)).any()
    # the borders: left-hand side one above, at and one below the right-hand side
    border = recs[19:22]
    assert border["samples"].tolist() == [2, 2, 2]
    assert m.adapt_active(border, m.make_adapt_params(2, 0xFFFFFFFF, 1)).tolist() == [True, False, False]
    # sums at 2^56 - 1: the products pass 64 bits
    big = recs[16:18]
    assert int(big["sum"][0, 0]) == (1 << 56) - 1
    assert m.adapt_active(big, m.make_adapt_params(4, 32, 65535)).tolist() == [True, True]      # e = m either way: 65536 m > 65535 (m + 2^21)
    assert m.adapt_active(big, m.make_adapt_params(4, 32, 65536)).tolist() == [False, False]


def test_the_rule_on_seeded_records_of_every_bit_pattern():
    rng = np.random.default_rng(16)
    recs = np.zeros(4096, ADAPT_PIXEL_DTYPE)
    raw = rng.integers(0, 1 << 63, (4096, 6), dtype=np.uint64) * 2 + rng.integers(0, 2, (4096, 6), dtype=np.uint64)     # all 64 bits in use
    raw >>= rng.integers(0, 64, (4096, 6)).astype(np.uint64)                                                              # ... and every magnitude
    recs["sum"], recs["even"] = raw[:, :3], raw[:, 3:]
    recs["samples"] = rng.integers(0, 1 << 32, 4096, dtype=np.uint64) >> rng.integers(0, 32, 4096).astype(np.uint64)
    seen = set()
    for case in ((0, 0xFFFFFFFF, 4096), (2, 0xFFFFFFFF, 0xFFFFFFFF), (0, 1 << 24, 1), (0, 0xFFFFFFFF, 70000)):
        seen.update(_agree(recs, case, "random bit patterns").tolist())
    assert seen == {True, False}
    # realistic records: sums of n samples, the even half near one half of them
    n = rng.integers(2, 1 << 24, 4096)
    s = (rng.integers(0, 1 << 32, (4096, 3)) * n[:, None]).astype(np.uint64)             # below 2^56
    recs["sum"], recs["even"], recs["samples"] = s, (s * rng.uniform(0.45, 0.55, (4096, 3))).astype(np.uint64), n
    for tol in (0, 1, 1024, 4096, 6000, 0xFFFFFFFF):
        _agree(recs, (4, 1 << 24, tol), "realistic records")


def test_null_pointers_of_the_host_rule():
    lib, px, ad, out = m.lib(), _abi.MirtAdaptPixel(), _abi.MirtAdaptParams(), C.c_uint32(7)
    assert lib.mirt_adapt_active(None, C.byref(ad), C.byref(out)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_adapt_active(C.byref(px), None, C.byref(out)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_adapt_active(C.byref(px), C.byref(ad), None) == _abi.MIRT_ERR_NULL_POINTER
    assert out.value == 7
    ad.max_samples = 1
    assert lib.mirt_adapt_active(C.byref(px), C.byref(ad), C.byref(out)) == 0 and out.value == 1


def test_every_error_path_that_needs_no_device():
    lib = m.lib()
    p, ad, st, n = ar.params(), m.make_adapt_params(4, 32, 4096), _abi.MirtAdaptStats(), C.c_uint32()
    buf = (C.c_uint8 * 256)()
    v = C.cast(buf, C.c_void_p)
    E = _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_adapt_reset(None, C.byref(p)) == E
    assert lib.mirt_ctx_adapt_step_device(None, C.byref(p), C.byref(ad), None) == E
    assert b"null" in lib.mirt_last_error()
    assert lib.mirt_ctx_adapt_resolve_device(None, C.byref(p), v, 256, None) == E
    assert lib.mirt_ctx_adapt_resolve(None, C.byref(p), v, 256) == E
    assert lib.mirt_ctx_adapt_read(None, v, 4) == E
    assert lib.mirt_ctx_adapt_write(None, v, 4) == E
    assert lib.mirt_ctx_adapt_list_read(None, v, 4, C.byref(n)) == E
    assert lib.mirt_ctx_adapt_stats(None, C.byref(st)) == E


def test_the_wrappers_check_their_arguments_before_the_library():
    with pytest.raises(ValueError):
        m.make_adapt_params(-1, 32, 4096)
    with pytest.raises(ValueError):
        m.make_adapt_params(4, 1 << 32, 4096)
    with pytest.raises(ValueError):
        m.make_adapt_params(4, 32, 0.5)
    with pytest.raises(ValueError):
        m.adapt_active(np.zeros(4, np.uint64), m.make_adapt_params(4, 32, 4096))
    with pytest.raises(ValueError):
        m.adapt_active(np.zeros(4, ADAPT_PIXEL_DTYPE), (4, 32, 4096))
    ctx = Context.__new__(Context)                   # no device: the wrappers refuse before they would touch the handle
    ctx._h = C.c_void_p()
    with pytest.raises(ValueError):
        ctx.adapt_step(ar.params(), (4, 32, 4096))
    with pytest.raises(ValueError):
        ctx.adapt_reset((48, 32))
    with pytest.raises(ValueError):
        ctx.adapt_write(np.zeros(4, np.uint64))
    assert callable(m.Raytracer.render_adaptive)


# ---- the replay's footing ----

def test_one_sample_frames_add_up_to_the_oracles_render():
    """8 one-sample frames equal one 8-spp oracle render: what makes frame s of sample_frames "every pixel's sample s"."""
    frames = ar.sample_frames(ar.scene(), ar.params(), 8, "field300")
    assert frames.shape == (8, ar.W * ar.H, 3) and frames.dtype == np.uint64
    whole = ob.render_pt_sums(ar.scene(), ar.params(spp=8)).reshape(-1, 3)
    assert np.array_equal(frames.sum(axis=0, dtype=np.uint64), whole)
    assert len(np.unique(frames.reshape(8, -1), axis=0)) == 8                  # eight different samples
    # ... and the replay of two steps of 4 with everything active is that render, with the even half the even frames' sum
    steps = ar.replay(frames, 4, 8, 8, 0, 3)
    assert [len(s["list"]) for s in steps] == [ar.W * ar.H, ar.W * ar.H, 0] and steps[-1]["total"] == 8 * ar.W * ar.H
    rec = steps[-1]["records"]
    assert np.array_equal(rec["sum"], whole) and np.array_equal(rec["even"], frames[0::2].sum(axis=0, dtype=np.uint64))
    assert (rec["samples"] == 8).all() and not rec["_pad0"].any() and not rec["_pad1"].any()


def test_the_reference_loop_is_the_one_the_input_was_chosen_for():
    steps = ar.reference_loop()                      # asserts its preconditions itself
    assert [len(s["list"]) for s in steps] == [1536, 731, 599, 486, 401, 333, 273, 243, 0]
    final = steps[-1]["records"]["samples"]
    assert [int((final == n).sum()) for n in range(4, 33, 4)] == [805, 132, 113, 85, 68, 60, 30, 243]
    assert steps[-1]["total"] == 18408 == int(final.sum())
    for s in steps:
        assert (np.diff(s["list"].astype(np.int64)) > 0).all()
