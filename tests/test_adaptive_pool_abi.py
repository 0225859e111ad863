"""MIRT_ADAPT_POOL through the layers that need no device: the constant across the header, the ctypes mirror, the package, the crate
and the C++ mirror, the unchanged version, mirt_adapt_pool_plan against a restatement of its formula and rule (and mirt_bvh_pool_plan
against its own, unchanged), the wrappers' argument checks and the refusals that come before any device call."""
import ctypes as C
import re
from pathlib import Path

import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
POOL = 2
KEYS = ("threads", "slots", "waves_per_cu", "stack_entries", "lds_bytes_per_block")


def test_the_constant_is_bit_1_in_an_enum_of_its_own():
    assert re.search(r"^enum \{ MIRT_ADAPT_POOL = 1u << 1 \};", HEADER, re.M)
    assert len(re.findall(r"\bMIRT_ADAPT_POOL = ", HEADER)) == 1
    assert _abi.MIRT_ADAPT_POOL == POOL == m.MIRT_ADAPT_POOL
    assert re.search(r"pub const MIRT_ADAPT_POOL: u32 = 1 << 1;", RS)
    assert re.search(r'#include "[./]*include/mirt.h"', HPP)                 # the C++ mirror takes the constant from the header ...
    assert re.search(r"static_assert\(MIRT_ADAPT_POOL == 1u << 1\b", HPP)     # ... and states its value
    # no layer gives bit 0 of MirtAdaptParams.flags a name
    assert not re.search(r"\bMIRT_ADAPT_\w+ = 1u << 0\b", HEADER) and not re.search(r"pub const MIRT_ADAPT_\w+: u32 = 1( << 0)?;", RS)
    assert [n for n in dir(_abi) if n.startswith("MIRT_ADAPT_") and getattr(_abi, n) == 1] == []


def test_the_version_is_unchanged():
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0    # a new flag and a new host-only export, no new version


def test_the_export_exists_with_four_arguments():
    proto = re.search(r"^int mirt_adapt_pool_plan\(([^)]*)\);", HEADER, re.M)
    assert proto and [a.strip() for a in proto.group(1).split(",")] == \
        ["uint32_t max_depth", "uint32_t hosek", "uint64_t lds_bytes_per_cu", "MirtBvhPoolPlan* out"]
    assert _abi.SYMBOLS["mirt_adapt_pool_plan"] == _abi.SYMBOLS["mirt_bvh_pool_plan"] and len(_abi.SYMBOLS["mirt_adapt_pool_plan"][1]) == 4
    f = m.lib().mirt_adapt_pool_plan                            # the library exports it
    assert f.restype is C.c_int and list(f.argtypes) == list(_abi.SYMBOLS["mirt_adapt_pool_plan"][1])
    assert re.search(r"pub fn mirt_adapt_pool_plan\(max_depth: u32, hosek: u32, lds_bytes_per_cu: u64, out: \*mut MirtBvhPoolPlan\) -> c_int;", RS)
    assert re.search(r"\bmirt_adapt_pool_plan\(max_depth, hosek \? 1u : 0u, lds_bytes_per_cu, &plan\)", HPP)


def _plan(max_depth, hosek, lds, per_wave):
    """include/mirt.h restated: 256 threads; of 112, 96, 80 and 64 slots the largest that leaves 16 waves resident per compute unit,
    else the one that keeps most waves, the larger pools on a tie; per_wave = the bytes a wave keeps beside its 50 x slots and its stacks."""
    best = dict.fromkeys(KEYS, 0)
    for slots in (112, 96, 80, 64):
        block = 96 + (144 if hosek else 0) + 4 * (50 * slots + per_wave + 256 * max_depth)
        waves = 4 * min(lds // block, 4)
        if waves > best["waves_per_cu"]:
            best = dict(threads=256, slots=slots, waves_per_cu=waves, stack_entries=max_depth, lds_bytes_per_block=block)
        if waves == 16:
            break
    return best


@pytest.mark.parametrize("lds", [163840, 65536])
@pytest.mark.parametrize("hosek", [False, True], ids=["no sky", "hosek"])
def test_the_plan_follows_its_formula_and_the_parents_plan_is_unchanged(hosek, lds):
    for depth in range(0, 33):
        assert m.adapt_pool_plan(depth, hosek, lds) == _plan(depth, hosek, lds, 896), (depth, hosek, lds)
        assert m.bvh_pool_plan(depth, hosek, lds) == _plan(depth, hosek, lds, 384), (depth, hosek, lds)
    if lds == 163840:                                            # 0 = gfx950's 163 840
        for depth in (0, 9, 20, 32):
            assert m.adapt_pool_plan(depth, hosek) == m.adapt_pool_plan(depth, hosek, lds)


def test_the_plans_the_contract_names():
    assert tuple(m.adapt_pool_plan(9)[k] for k in KEYS) == (256, 112, 16, 9, 35296)
    assert tuple(m.adapt_pool_plan(32)[k] for k in KEYS) == (256, 80, 12, 32, 52448)
    # at depth 32, 96 and 112 slots keep 8 waves, 80 and 64 keep 12: the larger pool wins the tie
    per_block = {s: 96 + 4 * (50 * s + 896 + 256 * 32) for s in (112, 96, 80, 64)}
    assert {s: 4 * min(163840 // b, 4) for s, b in per_block.items()} == {112: 8, 96: 8, 80: 12, 64: 12}
    # the largest depth that still runs 112 slots at 16 waves is 14
    assert [d for d in range(33) if m.adapt_pool_plan(d)["slots"] == 112 and m.adapt_pool_plan(d)["waves_per_cu"] == 16][-1] == 14
    assert m.adapt_pool_plan(15)["slots"] < 112


def test_the_plans_refusals():
    lib = m.lib()
    out = _abi.MirtBvhPoolPlan()
    assert lib.mirt_adapt_pool_plan(9, 0, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    out.slots = 7
    assert lib.mirt_adapt_pool_plan(33, 0, 0, C.byref(out)) == _abi.MIRT_ERR_BAD_ROWS == lib.mirt_bvh_pool_plan(33, 0, 0, C.byref(out))
    assert out.as_dict() == dict.fromkeys(KEYS, 0)
    assert lib.mirt_adapt_pool_plan(32, 1, 0, C.byref(out)) == _abi.MIRT_OK and out.slots == 80
    assert m.adapt_pool_plan(9, lds_bytes_per_cu=4096) == dict.fromkeys(KEYS, 0)      # not one block fits


@pytest.mark.parametrize("pool", [1, None, POOL, "yes", 0], ids=["1", "None", "the flag itself", "str", "0"])
def test_the_wrappers_refuse_a_pool_that_is_no_bool(pool):
    with pytest.raises(ValueError, match="pool must be a bool"):
        m.make_adapt_params(4, 32, 4096, pool)
    with pytest.raises(ValueError, match="pool must be a bool"):
        m.make_adapt_params(4, 32, 4096, pool=pool)
    # Raytracer.render_adaptive builds its params before it touches a context
    with pytest.raises(ValueError, match="pool must be a bool"):
        m.Raytracer.render_adaptive(object(), 4096, 32, pool=pool)


def test_the_wrapper_sets_the_bit():
    import numpy as np
    assert m.make_adapt_params(4, 32, 4096).flags == 0 == m.make_adapt_params(4, 32, 4096, False).flags
    a = m.make_adapt_params(4, 32, 4096, pool=True)
    assert (a.min_samples, a.max_samples, a.tolerance, a.flags) == (4, 32, 4096, POOL)
    assert m.make_adapt_params(4, 32, 4096, np.bool_(True)).flags == POOL


def test_a_null_context_with_the_flag_is_refused_before_any_device_call():
    lib = m.lib()
    p = m.make_params(8, 8, 4, mode=m.MIRT_MODE_PT)
    for flags in (POOL, POOL | 1, POOL | 4, 1, 3):
        a = m.make_adapt_params(4, 32, 4096)
        a.flags = flags
        assert lib.mirt_ctx_adapt_step_device(None, C.byref(p), C.byref(a), None) == _abi.MIRT_ERR_NULL_POINTER
