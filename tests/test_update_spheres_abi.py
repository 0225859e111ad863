"""mirt_ctx_update_spheres, mirt_ctx_update_spheres_device, mirt_ctx_bvh_refits and mirt_node_update_spheres through the layers that
need no device: the library's exports and its checks before any HIP call, the ctypes mirror, the Rust crate's source and the Python
wrappers' argument checks."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, SPHERE_DTYPE, sphere_records
from weekend_raytracer_wgpu_amd.node import Node

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
NEW = ("mirt_ctx_update_spheres", "mirt_ctx_update_spheres_device", "mirt_ctx_bvh_refits", "mirt_node_update_spheres")


def test_the_library_exports_the_four_symbols():
    lib = m.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.SYMBOLS, name


def test_a_null_context_is_refused_before_any_device_call():
    lib = m.lib()
    one = (_abi.MirtSphere * 1)()
    for count, ptr in ((1, C.cast(one, C.c_void_p)), (0, None), (1, None)):
        assert lib.mirt_ctx_update_spheres(None, 0, count, ptr) == _abi.MIRT_ERR_NULL_POINTER
        assert lib.mirt_ctx_update_spheres_device(None, 0, count, ptr) == _abi.MIRT_ERR_NULL_POINTER
        assert lib.mirt_node_update_spheres(None, 0, count, ptr) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_bvh_refits(None) == 0


def _arity(decl_args: str) -> int:
    return len([a for a in decl_args.split(",") if a.strip()])


def test_the_rust_source_declares_them_with_the_headers_arity():
    for name in NEW:
        h = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, HEADER)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, RS)
        assert h and r, name
        assert _arity(h.group(1)) == _arity(r.group(1)) == len(_abi.SYMBOLS[name][1]), name
    assert re.search(r"pub fn mirt_ctx_bvh_refits\([^)]*\) -> u32;", RS)
    assert _abi.SYMBOLS["mirt_ctx_bvh_refits"][0] is C.c_uint32


def test_the_wire_record():
    assert SPHERE_DTYPE.itemsize == C.sizeof(_abi.MirtSphere) == 32
    assert SPHERE_DTYPE.fields["radius"][1] == _abi.MirtSphere.radius.offset
    assert SPHERE_DTYPE.fields["material_idx"][1] == _abi.MirtSphere.material_idx.offset
    assert m.SPHERE_DTYPE is SPHERE_DTYPE


def test_sphere_records_accepts_the_three_forms():
    arr = np.zeros(5, SPHERE_DTYPE)
    ptr, count, keep = sphere_records(arr)
    assert count == 5 and ptr.value == keep.ctypes.data
    ptr, count, _ = sphere_records(arr[::2])                   # a strided view is gathered
    assert count == 3
    ptr, count, _ = sphere_records(np.zeros(0, SPHERE_DTYPE))
    assert count == 0
    carr = (_abi.MirtSphere * 4)()
    ptr, count, _ = sphere_records(carr)
    assert count == 4 and ptr.value == C.addressof(carr)
    ptr, count, keep = sphere_records([m.Sphere((1, 2, 3), 0.5, 7), m.Sphere((4, 5, 6), 2.0, 0).to_c()])
    assert count == 2 and keep[0].radius == 0.5 and list(keep[1].center)[:3] == [4.0, 5.0, 6.0]


class _NoLibrary:
    """A Context / Node whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.mark.parametrize("bad", [np.zeros((4, 8), np.float32), np.zeros(4, np.float64), np.zeros((2, 2), SPHERE_DTYPE),
                                 (C.c_float * 8)(), [1.0, 2.0], "spheres", None, 3, [object()]],
                         ids=["f32 matrix", "f64", "2-d records", "ctypes floats", "floats", "str", "None", "int", "objects"])
def test_the_wrappers_refuse_a_wrong_dtype_or_shape(bad, monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod, node as node_mod
    for mod in (context_mod, node_mod):
        monkeypatch.setattr(mod, "lib", lambda: pytest.fail("the library was called"), raising=True)
    with pytest.raises(ValueError):
        sphere_records(bad)
    with pytest.raises(ValueError):
        Context.update_spheres(_NoLibrary(), 0, bad)
    with pytest.raises(ValueError):
        Node.update_spheres(_NoLibrary(), 0, bad)


@pytest.mark.parametrize("first, count", [(-1, 1), (0, -1), (2 ** 32, 1), (0, 2 ** 32), (1.5, 1), (0, "2")])
def test_the_wrappers_refuse_a_range_that_is_no_u32(first, count):
    with pytest.raises(ValueError):
        Context.update_spheres_device(_NoLibrary(), first, count, 0x1000)
    if isinstance(count, int) and count == 1:
        with pytest.raises(ValueError):
            Context.update_spheres(_NoLibrary(), first, np.zeros(1, SPHERE_DTYPE))


def test_move_spheres_checks_its_range_and_keeps_materials():
    from weekend_raytracer_wgpu_amd.raytracer import _moved
    held = [m.Sphere((i, 0, 0), 1.0, i) for i in range(4)]
    for first in (1, np.int64(1), np.uint32(1)):                   # what Context.update_spheres takes as `first`
        at, out = _moved(held, first, [m.Sphere((9, 9, 9), 2.0, 77), m.Sphere((8, 8, 8), 3.0, 78)])
        assert at == 1 and type(at) is int
        assert [(s.center.tolist(), s.radius, s.material_idx) for s in out] == [([9.0, 9.0, 9.0], 2.0, 1), ([8.0, 8.0, 8.0], 3.0, 2)]
    for first, k in ((3, 2), (-1, 1), (5, 0), (1.0, 1), (True, 1)):
        with pytest.raises(ValueError):
            _moved(held, first, [m.Sphere((0, 0, 0), 1.0, 0)] * k)
    with pytest.raises(ValueError):
        _moved(held, 0, [held[0].to_c()])


class _Target:
    """Stands for a Context / Node in move_spheres: records the calls, fails on demand."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], fail

    def update_spheres(self, first, spheres):
        self.calls.append(("update", first, len(spheres)))
        if self.fail is not None:
            raise m.MirtError(self.fail, "injected")

    def set_scene(self, scene, **kw):
        self.calls.append(("set_scene", len(scene.spheres), kw))
        if self.fail is not None:
            raise m.MirtError(self.fail, "injected")

    def render(self, params):
        self.calls.append(("render", params.width, params.height, params.spp))
        return np.zeros((params.height, params.width, 4), np.uint8)

    def stats(self):
        return {}


def _layer(target, hbm):
    rp = m.RenderParams(camera=m.FlyCameraController.default().renderer_camera(), viewport_size=(8, 6))
    world = [m.Sphere((i, 0, 0), 1.0, i % 3) for i in range(6)]
    mats = [m.Material.Lambertian(albedo=m.Texture.new_from_color((0.5, 0.5, 0.5))) for _ in range(3)]
    layer = m.Layer.new([8, 6], rp, scene=m.Scene(world, mats))
    layer.set_global_data()
    layer._ctx, layer._hbm = target, hbm
    return layer, rp


def test_layer_move_spheres_picks_the_update_or_set_scene_and_renders():
    new = [m.Sphere((7, 7, 7), 2.0, 99)]
    layer, rp = _layer(None, False)                                 # nothing resident: only `world` changes
    layer.move_spheres(2, new, rp)
    assert layer.world[2].radius == 2.0 and layer.world[2].material_idx == 2 and layer._rgba is None
    t = _Target()
    layer, rp = _layer(t, True)                                     # an HBM scene: in place
    layer.move_spheres(np.int64(2), new, rp)
    assert t.calls == [("update", 2, 1), ("render", 8, 6, rp.sampling.num_samples_per_pixel)]
    assert layer.world[2].center.tolist() == [7.0, 7.0, 7.0] and layer._rgba.shape == (6, 8, 4)
    t = _Target()
    layer, rp = _layer(t, False)                                    # an LDS scene: set again, with the moved world
    layer.move_spheres(2, new)
    assert t.calls == [("set_scene", 6, {})] and layer.world[2].radius == 2.0 and layer._hbm is False


@pytest.mark.parametrize("status, keeps_hbm", [(_abi.MIRT_ERR_BAD_ROWS, True), (_abi.MIRT_ERR_HIP, False), (_abi.MIRT_ERR_NO_SCENE, False)])
def test_a_failed_move_leaves_the_held_scene_alone(status, keeps_hbm):
    new = [m.Sphere((7, 7, 7), 2.0, 99)]
    layer, rp = _layer(_Target(fail=status), True)
    with pytest.raises(m.MirtError):
        layer.move_spheres(2, new, rp)
    assert layer.world[2].radius == 1.0 and layer._hbm is keeps_hbm    # after a lost scene the next move sets it again
    layer, rp = _layer(_Target(fail=status), False)
    with pytest.raises(m.MirtError):
        layer.move_spheres(2, new)
    assert layer.world[2].radius == 1.0
    rt = m.Raytracer.__new__(m.Raytracer)                           # the same rule in Raytracer.move_spheres, without a device
    rt.spheres = [m.Sphere((i, 0, 0), 1.0, 0) for i in range(4)]
    rt._ctx, rt._hbm, rt._accumulated = _Target(fail=status), True, 3
    with pytest.raises(m.MirtError):
        rt.move_spheres(1, new)
    assert rt.spheres[1].radius == 1.0 and rt._hbm is keeps_hbm and rt._accumulated == 3
