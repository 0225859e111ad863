"""MIRT_SCENE_BVH_DEVICE, MirtBvhInfo and the two mirt_ctx_bvh_* entry points through the layers that need no device: the header, the
ctypes mirror, the Rust crate's source and the Python wrappers' argument checks."""
import ctypes as C
import re
from pathlib import Path

import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import scene_flags

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()


def test_the_flag_has_one_value_everywhere():
    value = eval(re.search(r"MIRT_SCENE_BVH_DEVICE\s*=\s*([^,/\n]+)", HEADER).group(1).strip().replace("u", ""))
    assert value == 2 == _abi.MIRT_SCENE_BVH_DEVICE == m.MIRT_SCENE_BVH_DEVICE
    assert eval(re.search(r"pub const MIRT_SCENE_BVH_DEVICE: u32 = ([^;]+);", RS).group(1)) == value
    assert _abi.MIRT_SCENE_HBM == 1                       # the two flags are different bits


def test_bvh_info_layout_and_the_rust_struct():
    I = _abi.MirtBvhInfo
    assert C.sizeof(_abi.MirtBvhPlan) == 32 and C.sizeof(I) == 64
    assert (I.plan.offset, I.root.offset, I.built_on_device.offset, I.centre.offset, I.radius.offset, I.r_max.offset) == (0, 32, 36, 40, 52, 56)
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct MirtBvhInfo \{(.*?)\n\}", RS, re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,\n]+),", body) == [("plan", "MirtBvhPlan"), ("root", "u32"), ("built_on_device", "u32"),
                                                          ("centre", "[f32; 3]"), ("radius", "f32"), ("r_max", "f32")]
    fields = re.search(r"typedef struct MirtBvhInfo \{(.*?)\} MirtBvhInfo;", HEADER, re.S).group(1)
    names = re.findall(r"\b(plan|root|built_on_device|centre|radius|r_max)\b(?=[\[;,])", fields)
    assert names == [f[0] for f in I._fields_]


def test_the_library_exports_the_entry_points():
    lib = m.lib()
    for name in ("mirt_ctx_bvh_info", "mirt_ctx_bvh_read"):
        assert hasattr(lib, name) and name in _abi.SYMBOLS
    out = _abi.MirtBvhInfo()
    assert lib.mirt_ctx_bvh_info(None, C.byref(out)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_bvh_read(None, None, 0, None, 0, None, 0) == _abi.MIRT_ERR_NULL_POINTER


def test_scene_flags():
    assert scene_flags(False, "host") == 0
    assert scene_flags(True, "host") == _abi.MIRT_SCENE_HBM
    assert scene_flags(True, "device") == _abi.MIRT_SCENE_HBM | _abi.MIRT_SCENE_BVH_DEVICE
    with pytest.raises(ValueError):
        scene_flags(False, "device")                      # the C ABI answers MIRT_ERR_BAD_MODE; the wrapper says why
    with pytest.raises(ValueError):
        scene_flags(True, "gpu")
