"""The progressive-frame entry points (mirt_ctx_accum_frame*, mirt_node_accum_*) without a GPU: the library exports them, and a
null context or node is refused before any device is touched."""
import ctypes as C

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi

NEW_SYMBOLS = ["mirt_ctx_accum_frame_device", "mirt_ctx_accum_frame", "mirt_node_accum_reset", "mirt_node_accum_frame_device",
               "mirt_node_accum_frame", "mirt_node_accum_samples", "mirt_node_accum_read"]


def _params():
    return m.make_params(64, 48, 2, mode=m.MIRT_MODE_PT, num_bounces=8)


def test_library_exports_the_seven_symbols():
    raw = C.CDLL(str(m.LIB_PATH))                     # a fresh handle: no argtypes attached, only the dynamic symbol table counts
    missing = [name for name in NEW_SYMBOLS if not hasattr(raw, name)]
    assert not missing, missing
    assert all(name in _abi.SYMBOLS for name in NEW_SYMBOLS)


def test_null_context_is_refused_before_any_device_is_touched():
    lib, p = m.lib(), _params()
    host = (C.c_uint8 * (64 * 48 * 4))()
    # a non-null "device" address that is never dereferenced: the context is checked first
    assert lib.mirt_ctx_accum_frame_device(None, C.byref(p), C.cast(host, C.c_void_p), len(host), None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_last_error()
    assert lib.mirt_ctx_accum_frame(None, C.byref(p), C.cast(host, C.c_void_p), len(host)) == _abi.MIRT_ERR_NULL_POINTER


def test_null_node_is_refused_before_any_device_is_touched():
    lib, p = m.lib(), _params()
    host = (C.c_uint8 * (64 * 48 * 4))()
    sums = (C.c_uint64 * (64 * 48 * 3))()
    assert lib.mirt_node_accum_reset(None, C.byref(p)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_frame_device(None, C.byref(p), C.cast(host, C.c_void_p), len(host), None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_frame(None, C.byref(p), C.cast(host, C.c_void_p), len(host)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_read(None, C.cast(sums, C.c_void_p), len(sums)) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_samples(None) == 0


def test_null_params_and_outputs_are_refused_too():
    """Still without a device: a node handle cannot exist here, so only the argument order of the checks is visible -- a null
    params pointer with a null handle is MIRT_ERR_NULL_POINTER, never a crash."""
    lib = m.lib()
    assert lib.mirt_ctx_accum_frame_device(None, None, None, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_accum_frame(None, None, None, 0) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_reset(None, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_frame_device(None, None, None, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_frame(None, None, None, 0) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_node_accum_read(None, None, 0) == _abi.MIRT_ERR_NULL_POINTER
