"""Node: one process renders one frame on several devices through the C ABI (mirt_node_*, include/mirt.h).

Member i of a node renders its share of the 4-row tile interleave; the parts are assembled on member 0.  Every entry of
`devices` naming one device -> loopback (parts read in place, no copies); all entries distinct -> RCCL gather (`rccl=True`
forces it, also for one device).  The image is byte-identical to `Context.render` of the same params.  No torch needed."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._lib import check, lib
from .context import Context, SceneData, _check_range, _stream_arg, params_out_rows, scene_flags, sphere_records


class _MemberContext(Context):
    """A member's context, borrowed from its node: the Context methods work on it; closing it is a no-op (the node owns it)."""

    def __init__(self, handle: C.c_void_p, device: int, node: "Node"):
        self._h = handle
        self.device = device
        self._scene = None
        self._node = node            # keeps the node (and so the context) alive while this wrapper is

    def close(self) -> None:
        pass


class Node:
    """mirt_node_* : member contexts on `devices`, one frame assembled on member 0."""

    def __init__(self, devices: Sequence[int], rccl: bool = False):
        devs = [int(d) for d in devices]
        arr = (C.c_int * max(1, len(devs)))(*devs)
        self._h = C.c_void_p()
        check(lib().mirt_node_create(arr, len(devs), _abi.MIRT_NODE_RCCL if rccl else 0, C.byref(self._h)))
        self.devices = devs
        self._scene: Optional[SceneData] = None

    def close(self) -> None:
        if self._h:
            lib().mirt_node_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self) -> "Node":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, scene: SceneData, *, hbm: bool = False, bvh: str = "host") -> None:
        """mirt_node_set_scene; hbm=True: mirt_node_set_scene_ex(MIRT_SCENE_HBM) on every member (Context.set_scene); bvh="device":
        | MIRT_SCENE_BVH_DEVICE, every member builds its own tree on its own device."""
        flags = scene_flags(hbm, bvh)
        c = scene.as_c()
        if flags:
            check(lib().mirt_node_set_scene_ex(self._h, C.byref(c), flags))
        else:
            check(lib().mirt_node_set_scene(self._h, C.byref(c)))
        self._scene = scene

    def update_spheres(self, first: int, spheres) -> None:
        """mirt_node_update_spheres: Context.update_spheres on every member (host records only)."""
        ptr, count, keep = sphere_records(spheres)
        _check_range(first, count)
        check(lib().mirt_node_update_spheres(self._h, int(first), count, ptr))
        del keep

    def set_spheres(self, spheres) -> None:
        """mirt_node_set_spheres: Context.set_spheres on every member (host records only)."""
        ptr, count, keep = sphere_records(spheres)
        _check_range(0, count)
        check(lib().mirt_node_set_spheres(self._h, ptr, count))
        del keep

    def set_camera(self, camera: _abi.MirtGpuCamera) -> None:
        check(lib().mirt_node_set_camera(self._h, C.byref(camera)))

    def render(self, params: _abi.MirtParams) -> np.ndarray:
        """Render the band to host memory -> uint8 [rows, width, 4]; `params` carries no partition (tile_rows = n_parts = part = 0)."""
        rows = params_out_rows(params)
        out = np.empty((max(rows, 0), params.width, 4), dtype=np.uint8)
        check(lib().mirt_node_render(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def render_device(self, params: _abi.MirtParams, d_ptr: int, nbytes: int, stream: Optional[int] = None) -> None:
        """Render asynchronously into device memory on member 0's device, ordered on `stream` (None = the node's own stream; the
        default stream, 0, is refused by the library: pass a stream of your own)."""
        check(lib().mirt_node_render_device(self._h, C.byref(params), C.c_void_p(d_ptr), nbytes, _stream_arg(stream)))

    # ---- progressive accumulation: every member owns the exact sums of its part; a frame moves RGBA8 parts only ----
    def accum_reset(self, params: _abi.MirtParams) -> None:
        check(lib().mirt_node_accum_reset(self._h, C.byref(params)))

    def accum_frame_device(self, params: _abi.MirtParams, d_out: int, stream: Optional[int] = None, nbytes: Optional[int] = None) -> None:
        """mirt_node_accum_frame_device: one progressive frame of the band (Context.accum_frame_device on every member, then the
        node's gather and assembly) into device memory at address `d_out` on member 0's device, ordered on `stream`."""
        if nbytes is None:
            nbytes = params_out_rows(params) * params.width * 4
        check(lib().mirt_node_accum_frame_device(self._h, C.byref(params), C.c_void_p(d_out), nbytes, _stream_arg(stream)))

    def accum_frame(self, params: _abi.MirtParams) -> np.ndarray:
        """The same frame to host memory (blocking) -> uint8 [rows, width, 4]."""
        out = np.empty((params_out_rows(params), params.width, 4), dtype=np.uint8)
        check(lib().mirt_node_accum_frame(self._h, C.byref(params), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def accum_samples(self) -> int:
        return int(lib().mirt_node_accum_samples(self._h))

    def accum_read(self, params: _abi.MirtParams) -> np.ndarray:
        """The band's sums in band-row order -> uint64 [rows, width, 3]."""
        out = np.empty((params_out_rows(params), params.width, 3), dtype=np.uint64)
        check(lib().mirt_node_accum_read(self._h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def context(self, i: int) -> Context:
        """Member i's context (borrowed): stats(), last_kernel(), set_timing()."""
        h = C.c_void_p()
        check(lib().mirt_node_context(self._h, i, C.byref(h)))
        return _MemberContext(h, self.devices[i], self)

    def stats(self) -> dict:
        st = _abi.MirtNodeStats()
        check(lib().mirt_node_get_stats(self._h, C.byref(st)))
        return st.as_dict()
