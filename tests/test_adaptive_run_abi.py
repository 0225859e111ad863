"""mirt_ctx_adapt_run_* through the layers that need no device: exports, arities, the two structs and the constant across the header, the
ctypes mirror, the C++ mirror and the Rust crate's source; mirt_adapt_run_spp -- the function the scan stage runs on the device --
against the rule in Python's unlimited integers (tests/adaptive_run_ref.py) at its corners and on seeded triples; every refusal that
needs no device; and the reference runs' own preconditions."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd._lib import MirtError
from weekend_raytracer_wgpu_amd.context import Context
import adaptive_ref as ar
import adaptive_run_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
NEW = {"mirt_adapt_run_spp": 4, "mirt_ctx_adapt_run_device": 5, "mirt_ctx_adapt_run_read": 4}
STRUCTS = {"MirtAdaptRun": 16, "MirtAdaptRunStep": 8}
MAX_SPP = _abi.MIRT_MAX_SPP_PER_CALL


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


def test_struct_layouts_and_the_constant():
    R, S = _abi.MirtAdaptRun, _abi.MirtAdaptRunStep
    assert (C.sizeof(R), C.sizeof(S)) == (16, 8)
    assert (R.max_steps.offset, R.min_items.offset, R.max_spp.offset, R.flags.offset) == (0, 4, 8, 12)
    assert (S.count.offset, S.spp.offset) == (0, 4)
    for name, size in STRUCTS.items():
        assert re.search(r"static_assert\(sizeof\(%s\) == %d," % (name, size), HEADER), name
        assert re.search(r"_Static_assert\(sizeof\(%s\) == %d," % (name, size), HEADER), name
        assert re.search(r"sizeof\(%s\) == %d" % (name, size), HPP), name
        assert re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^\]]*\)\]\s*)?pub struct %s " % name, RS), name
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, RS, re.S).group(1)
        assert re.findall(r"pub (\w+): u32,", body) == [f[0] for f in getattr(_abi, name)._fields_], name
        assert all(f[1] is C.c_uint32 for f in getattr(_abi, name)._fields_)
    assert re.search(r"typedef struct MirtAdaptRun\s+\{ uint32_t max_steps, min_items, max_spp, flags; \} MirtAdaptRun;", HEADER)
    assert re.search(r"typedef struct MirtAdaptRunStep \{ uint32_t count, spp; \} MirtAdaptRunStep;", HEADER)
    assert re.search(r"#define MIRT_ADAPT_RUN_MAX_STEPS 256u", HEADER)
    assert re.search(r"pub const MIRT_ADAPT_RUN_MAX_STEPS: u32 = 256;", RS)
    assert re.search(r"MIRT_ADAPT_RUN_MAX_STEPS == 256u", HPP)
    assert _abi.MIRT_ADAPT_RUN_MAX_STEPS == 256 == m.MIRT_ADAPT_RUN_MAX_STEPS
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0                # a new capability, no new version


# ---- the rule: mirt_adapt_run_spp against Python's integers ----

def _agree(count, spp, min_items, max_spp):
    got = m.adapt_run_spp(count, spp, m.make_adapt_run(1, min_items, max_spp))
    want = rr.run_spp(count, spp, min_items, max_spp)
    assert got == want, f"count {count}, spp {spp}, min_items {min_items}, max_spp {max_spp}: library {got}, rule {want}"
    return got


def test_the_rule_at_its_corners():
    # count x spp one below, at and one above min_items: the step doubles exactly when the product is below
    assert [_agree(100, 4, mi, 64) for mi in (401, 400, 399)] == [8, 4, 4]
    assert [_agree(100, 4, mi, 64) for mi in (801, 800, 799)] == [16, 8, 8]
    # the cap reached exactly, with the product still below min_items; a cap that is the base; cap 0 means the base
    assert _agree(3, 4, 1 << 20, 64) == 64 and _agree(3, 4, 3 * 64, 64) == 64 and _agree(3, 4, 3 * 64 + 1, 64) == 64 and _agree(3, 4, 3 * 32, 64) == 32
    assert _agree(3, 4, 1 << 20, 4) == 4 and _agree(3, 4, 1 << 20, 0) == 4
    # count 0: no samples, whatever the rest
    assert _agree(0, 4, 0, 0) == 0 and _agree(0, 4, 0xffffffff, 64) == 0 and _agree(0, MAX_SPP, 1, MAX_SPP) == 0
    # min_items 0 never grows
    assert _agree(1, 2, 0, MAX_SPP) == 2 and _agree(0xffffffff, 6, 0, 6 << 20) == 6
    # the 64-bit product: (2^32 - 1) x 2^24 is far above any 32-bit min_items; in 32 bits it would be 0xff000000 and below this one
    assert _agree(0xffffffff, MAX_SPP, 0xffffffff, MAX_SPP) == MAX_SPP
    assert _agree(0xffffffff, 1 << 23, 0xffffffff, MAX_SPP) == 1 << 23
    assert _agree(1 << 31, 2, 0xffffffff, MAX_SPP) == 2 and _agree((1 << 31) - 1, 2, 0xffffffff, MAX_SPP) == 4      # 2^32 >= 2^32 - 1 > 2^32 - 2
    # the reference runs' logs
    for (_, min_items, cap), log in rr.RUNS.values():
        for count, spp in log:
            assert _agree(count, rr.BASE, min_items, cap) == spp


def test_the_rule_on_seeded_triples():
    rng = np.random.default_rng(18)
    sizes = set()
    for _ in range(4000):
        base = 2 * int(rng.integers(1, 1 << int(rng.integers(1, 12))))
        m_max = (MAX_SPP // base).bit_length() - 1
        cap = 0 if rng.integers(0, 8) == 0 else base << int(rng.integers(0, m_max + 1))
        count = int(rng.integers(0, 1 << 32, dtype=np.uint64) >> np.uint64(rng.integers(0, 32)))
        min_items = int(rng.integers(0, 1 << 32, dtype=np.uint64) >> np.uint64(rng.integers(0, 32)))
        got = _agree(count, base, min_items, cap)
        sizes.add((got // base).bit_length() if got else 0)
    assert len(sizes) > 8                                                    # no growth, every k up to several doublings, and 0


# ---- refusals ----

def test_refusals_of_the_host_rule():
    lib, out = m.lib(), C.c_uint32(7)
    run = m.make_adapt_run(1, 100, 16)
    assert lib.mirt_adapt_run_spp(5, 4, None, C.byref(out)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_adapt_run_spp(5, 4, C.byref(run), None) == _abi.MIRT_ERR_NULL_POINTER
    for spp in (0, 3, MAX_SPP + 2):
        assert lib.mirt_adapt_run_spp(5, spp, C.byref(run), C.byref(out)) == _abi.MIRT_ERR_SPP_RANGE, spp
    for cap in (2, 6, 12, 17, 2 * MAX_SPP):                                  # below the base, no power-of-two multiple, above the limit
        bad = m.make_adapt_run(1, 100, cap)
        assert lib.mirt_adapt_run_spp(5, 4, C.byref(bad), C.byref(out)) == _abi.MIRT_ERR_SPP_RANGE, cap
    bad = m.make_adapt_run(1, 100, 16)
    bad.flags = 1
    assert lib.mirt_adapt_run_spp(5, 4, C.byref(bad), C.byref(out)) == _abi.MIRT_ERR_BAD_MODE
    assert out.value == 7                                                    # a refused call writes nothing
    zero_steps = m.make_adapt_run(0, 100, 16)                                # max_steps is not the rule's business
    assert lib.mirt_adapt_run_spp(5, 4, C.byref(zero_steps), C.byref(out)) == 0 and out.value == 16


def test_every_error_path_that_needs_no_device():
    lib = m.lib()
    p, ad, run, n = ar.params(), m.make_adapt_params(4, 32, 4096), m.make_adapt_run(8, 3000, 16), C.c_uint32(9)
    buf = (C.c_uint8 * 2048)()
    v = C.cast(buf, C.c_void_p)
    E = _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_adapt_run_device(None, C.byref(p), C.byref(ad), C.byref(run), None) == E
    assert b"null" in lib.mirt_last_error()
    assert lib.mirt_ctx_adapt_run_read(None, v, 256, C.byref(n)) == E and n.value == 9


def test_the_wrappers_check_their_arguments_before_the_library():
    for bad in ((-1, 0, 0), (1, 1 << 32, 0), (1, 0, 0.5), (True, 0, 0)):
        with pytest.raises(ValueError):
            m.make_adapt_run(*bad)
    with pytest.raises(ValueError):
        m.adapt_run_spp(5, 4, (8, 3000, 16))
    with pytest.raises(ValueError):
        m.adapt_run_spp(-1, 4, m.make_adapt_run(1))
    with pytest.raises(MirtError):
        m.adapt_run_spp(5, 3, m.make_adapt_run(1))
    run = m.make_adapt_run(8)
    assert (run.max_steps, run.min_items, run.max_spp, run.flags) == (8, 0, 0, 0)
    ctx = Context.__new__(Context)                   # no device: the wrappers refuse before they would touch the handle
    ctx._h = C.c_void_p()
    with pytest.raises(ValueError):
        ctx.adapt_run(ar.params(), m.make_adapt_params(4, 32, 4096), (8, 3000, 16))
    with pytest.raises(ValueError):
        ctx.adapt_run(ar.params(), (4, 32, 4096), m.make_adapt_run(8))
    with pytest.raises(ValueError):
        ctx.adapt_run((48, 32), m.make_adapt_params(4, 32, 4096), m.make_adapt_run(8))
    import inspect
    assert inspect.signature(m.Raytracer.render_adaptive).parameters["run"].default is None


# ---- the reference runs ----

def test_the_reference_runs_are_the_ones_the_input_was_chosen_for():
    assert rr.reference_runs()                       # asserts its preconditions itself
    first = rr.reference_run("three sizes")
    assert first["log"].dtype == np.uint32 and first["log"].shape == (8, 2)
    assert [st["total"] for st in first["steps"]] == [6144, 11992, 16312, 19520, 24304, 24304, 24304, 24304]
    assert first["steps"][5]["list"] is not None and len(first["steps"][5]["list"]) == 0 and first["steps"][6]["list"] is None
    final = first["steps"][-1]["records"]
    assert int(final["samples"].sum()) == 24304 and not final["_pad0"].any() and not final["_pad1"].any()
    # a run that never grows is the host-driven loop of tests/adaptive_ref.py, step for step
    plain = rr.replay_run(rr.frames_of(), rr.BASE, rr.MIN_SAMPLES, rr.MAX_SAMPLES, rr.TOLERANCE, (ar.N_STEPS, 0, 0))
    for got, want in zip(plain["steps"], ar.reference_loop()):
        assert np.array_equal(got["list"], want["list"]) and got["total"] == want["total"]
        assert np.array_equal(got["records"].view(np.uint8), want["records"].view(np.uint8))
    assert plain["log"].tolist() == [[len(s["list"]), 4 if len(s["list"]) else 0] for s in ar.reference_loop()]
