"""MIRT_RADIANCE_POOL through the layers that need no device: the constant across the header, the ctypes mirror, the package, the
crate and the C++ mirror, the bits that stay unassigned, the unchanged version, the wrappers' argument checks and the refusals that
come before any device call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, RADIANCE_RAY_DTYPE

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
POOL = 1 << 6


def test_the_constant_is_bit_6_in_an_enum_of_its_own():
    assert re.search(r"^enum \{ MIRT_RADIANCE_POOL = 1u << 6 \};", HEADER, re.M)
    # the enum tests/test_ray_sort_abi.py reads still holds exactly its four names
    enum = re.search(r"enum \{ (MIRT_RADIANCE_FLAT[^}]*)\}", HEADER).group(1)
    names = dict((n, int(s)) for n, s in re.findall(r"(MIRT_\w+) = 1u << (\d+)", enum))
    assert names == {"MIRT_RADIANCE_FLAT": 0, "MIRT_RADIANCE_ACCUMULATE": 1, "MIRT_RADIANCE_SKY_HOSEK": 2, "MIRT_RADIANCE_SORT": 4}
    assert _abi.MIRT_RADIANCE_POOL == POOL == m.MIRT_RADIANCE_POOL
    assert re.search(r"pub const MIRT_RADIANCE_POOL: u32 = 1 << 6;", RS)
    assert re.search(r'#include "[./]*include/mirt.h"', HPP)                  # the C++ mirror takes the constant from the header ...
    assert re.search(r"static_assert\(MIRT_RADIANCE_POOL == 1u << 6\b", HPP)   # ... and states its value


def test_bits_3_and_5_stay_unassigned():
    header = dict((n, int(s)) for n, s in re.findall(r"\b(MIRT_RADIANCE_\w+) = 1u << (\d+)", HEADER))
    crate = dict((n, int(s)) for n, s in re.findall(r"pub const (MIRT_RADIANCE_\w+): u32 = 1 << (\d+);", RS))
    mirror = {n: getattr(_abi, n).bit_length() - 1 for n in dir(_abi) if n.startswith("MIRT_RADIANCE_")}
    assert header == crate == mirror and len(header) == 5
    for name, shift in header.items():
        assert 1 << shift not in (8, 32), name
        assert getattr(_abi, name) == 1 << shift == getattr(m, name)
    assert len(set(header.values())) == len(header)


def test_the_version_is_unchanged():
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0    # a new flag, no new version


class _NoLibrary:
    """A Context whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod
    monkeypatch.setattr(context_mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("pool", [1, None, POOL, "yes", 0], ids=["1", "None", "the flag itself", "str", "0"])
def test_the_wrappers_refuse_a_pool_that_is_no_bool(pool, no_library):
    with pytest.raises(ValueError, match="pool must be a bool"):
        Context.trace_radiance(_NoLibrary(), np.zeros(2, RADIANCE_RAY_DTYPE), 4, pool=pool)
    with pytest.raises(ValueError, match="pool must be a bool"):
        Context.trace_radiance_device(_NoLibrary(), 0x1000, 2, 0x2000, 4, pool=pool)


def test_the_wrappers_set_the_bit():
    from weekend_raytracer_wgpu_amd.context import _radiance_params
    assert _radiance_params(4, 0, 8, 0, False, False, False).flags == 0
    assert _radiance_params(4, 0, 8, 0, False, False, False, False, True).flags == POOL
    assert _radiance_params(4, 0, 8, 0, False, True, True, True, np.bool_(True)).flags == POOL | 4 | 2 | 16


def test_a_null_context_with_the_flag_is_refused_before_any_device_call():
    lib = m.lib()
    rays, out = (_abi.MirtRadianceRay * 2)(), (_abi.MirtRadiance * 2)()
    pr, po = C.cast(rays, C.c_void_p), C.cast(out, C.c_void_p)
    before = bytes(out)
    for flags in (POOL, POOL | _abi.MIRT_RADIANCE_SORT, POOL | 7, POOL | 8, POOL | 32):
        p = _abi.MirtRadianceParams(4, 0, 8, flags, 0)
        for n, a, b in ((2, pr, po), (0, None, None)):
            assert lib.mirt_ctx_trace_radiance(None, a, n, C.byref(p), b) == _abi.MIRT_ERR_NULL_POINTER
            assert lib.mirt_ctx_trace_radiance_device(None, a, n, C.byref(p), b, None) == _abi.MIRT_ERR_NULL_POINTER
    assert bytes(out) == before
