"""The node's C ABI (mirt_node_*) without a GPU: argument and device-list checks come before any HIP call, libmirt.so does
not link librccl, and MirtNodeStats / the node constants agree between include/mirt.h, the ctypes binding and the Rust crate."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()


def _create(devices, flags=0, *, null_list=False, null_out=False):
    arr = (C.c_int * max(1, len(devices)))(*devices)
    h = C.c_void_p()
    rc = m.lib().mirt_node_create(None if null_list else arr, len(devices), flags, None if null_out else C.byref(h))
    if rc == _abi.MIRT_OK:
        m.lib().mirt_node_destroy(h)
    return rc, m.lib().mirt_last_error().decode()


def test_null_arguments():
    assert _create([0], null_list=True)[0] == _abi.MIRT_ERR_NULL_POINTER
    assert _create([0], null_out=True)[0] == _abi.MIRT_ERR_NULL_POINTER


def test_bad_device_lists_are_refused_before_any_hip_call():
    cases = {
        "empty": ([], 0),
        "too many": ([0] * (_abi.MIRT_NODE_MAX_MEMBERS + 1), 0),
        "mixed": ([0, 1, 0], 0),
        "rccl on a repeated device": ([0, 0], _abi.MIRT_NODE_RCCL),
    }
    messages = {}
    for what, (devices, flags) in cases.items():
        rc, msg = _create(devices, flags)
        assert rc == _abi.MIRT_ERR_NO_DEVICE, (what, rc, msg)
        assert msg and "no CPU fallback" not in msg, (what, msg)
        messages[what] = msg
    assert len(set(messages.values())) == len(cases), messages
    assert "16" in messages["too many"] and "mixed" in messages["mixed"] and "RCCL" in messages["rccl on a repeated device"]


def test_valid_list_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        rc, msg = _create([0])
        assert rc == _abi.MIRT_OK, msg
        return
    for devices, flags in (([0], 0), ([0, 0, 0, 0], 0), ([0, 1], 0), ([0], _abi.MIRT_NODE_RCCL)):
        rc, msg = _create(devices, flags)
        assert rc == _abi.MIRT_ERR_NO_DEVICE and "no CPU fallback" in msg, (devices, flags, rc, msg)
    with pytest.raises(m.MirtError) as e:
        m.Node([0, 0])
    assert e.value.status == _abi.MIRT_ERR_NO_DEVICE


def test_library_does_not_link_rccl():
    readelf = shutil.which("readelf")
    assert readelf, "readelf (binutils) is needed to read libmirt.so's dynamic section"
    out = subprocess.run([readelf, "-d", str(m.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", out)
    assert needed, out
    assert not [n for n in needed if "rccl" in n], needed


_C_TYPES = {"uint32_t": (4, C.c_uint32, "u32"), "double": (8, C.c_double, "f64")}


def test_node_stats_layout_agrees_across_header_ctypes_and_rust():
    body = re.search(r"typedef struct MirtNodeStats \{(.*?)\} MirtNodeStats;", HEADER, re.S).group(1)
    header = []
    for ctype, names in re.findall(r"^\s*(uint32_t|double)\s+([a-z_, ]+);", body, re.M):
        header += [(n.strip(), ctype) for n in names.split(",")]
    offset, want = 0, []
    for name, ctype in header:                                   # natural alignment, as a C compiler lays it out
        size = _C_TYPES[ctype][0]
        offset = (offset + size - 1) // size * size
        want.append((name, ctype, offset))
        offset += size
    py = [(f, t) for f, t in _abi.MirtNodeStats._fields_]
    assert [n for n, _, _ in want] == [f for f, _ in py]
    for (name, ctype, off), (_, pytype) in zip(want, py):
        assert pytype is _C_TYPES[ctype][1], name
        assert getattr(_abi.MirtNodeStats, name).offset == off, name
    assert C.sizeof(_abi.MirtNodeStats) == 24
    rs = re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^\]]*\)\]\s*)?pub struct MirtNodeStats \{(.*?)\n\}", RS, re.S)
    assert rs, "MirtNodeStats is not a #[repr(C)] struct of the Rust crate"
    rust = re.findall(r"pub (\w+): ([^,\n]+),", rs.group(2))
    assert [(n, t.strip()) for n, t in rust] == [(n, _C_TYPES[c][2]) for n, c, _ in want]


def test_node_constants_agree_across_header_ctypes_and_rust():
    max_members = int(re.search(r"#define MIRT_NODE_MAX_MEMBERS (\d+)", HEADER).group(1))
    rccl = eval(re.search(r"^\s*MIRT_NODE_RCCL\s*=\s*([^,/\n]+)", HEADER, re.M).group(1).strip().replace("u", ""))
    assert (max_members, rccl) == (16, 1)
    assert (_abi.MIRT_NODE_MAX_MEMBERS, _abi.MIRT_NODE_RCCL) == (max_members, rccl)
    assert (m.MIRT_NODE_MAX_MEMBERS, m.MIRT_NODE_RCCL) == (max_members, rccl)
    assert eval(re.search(r"pub const MIRT_NODE_MAX_MEMBERS: u32 = ([^;]+);", RS).group(1)) == max_members
    assert eval(re.search(r"pub const MIRT_NODE_RCCL: u32 = ([^;]+);", RS).group(1)) == rccl
    assert re.search(r"#\[repr\(C\)\]\s*pub struct MirtNode \{\s*_private: \[u8; 0\],\s*\}", RS), "opaque MirtNode"


def test_node_python_class_needs_no_torch():
    src = (ROOT / "weekend-raytracer-wgpu_amd" / "node.py").read_text()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)
