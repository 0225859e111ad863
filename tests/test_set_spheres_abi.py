"""mirt_ctx_set_spheres, mirt_ctx_set_spheres_device and mirt_node_set_spheres through the layers that need no device: the library's
exports and its checks before any HIP call, the ctypes mirror, the Rust crate's source, the Python wrappers' argument checks, the
choice Layer.set_world / Raytracer.set_world make -- and an audit of the always-list worlds the GPU tests use, by the host rule alone."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import Context, SPHERE_DTYPE
from weekend_raytracer_wgpu_amd.node import Node
import bvh_check
from hbm_worlds import c_spheres
from set_spheres_worlds import ALWAYS_WORLDS, shared_cap_expected

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
NEW = ("mirt_ctx_set_spheres", "mirt_ctx_set_spheres_device", "mirt_node_set_spheres")


def test_the_library_exports_the_three_symbols():
    lib = m.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in _abi.SYMBOLS, name


def test_a_null_context_or_node_is_refused_before_any_device_call():
    lib = m.lib()
    one = (_abi.MirtSphere * 1)()
    for ptr, count in ((C.cast(one, C.c_void_p), 1), (None, 0), (None, 1), (C.cast(one, C.c_void_p), 0)):
        for name in NEW:
            assert getattr(lib, name)(None, ptr, count) == _abi.MIRT_ERR_NULL_POINTER, (name, count)


def _arity(decl_args: str) -> int:
    return len([a for a in decl_args.split(",") if a.strip()])


def test_the_rust_source_and_the_ctypes_mirror_declare_them_with_the_headers_arity():
    for name in NEW:
        h = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, HEADER)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, RS)
        assert h and r, name
        assert _arity(h.group(1)) == _arity(r.group(1)) == len(_abi.SYMBOLS[name][1]) == 3, name
        assert _abi.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]), name


class _NoLibrary:
    """A Context / Node whose handle is never created: a wrapper that reached the library would dereference None."""
    _h = None


@pytest.fixture
def no_library(monkeypatch):
    from weekend_raytracer_wgpu_amd import context as context_mod, node as node_mod
    for mod in (context_mod, node_mod):
        monkeypatch.setattr(mod, "lib", lambda: pytest.fail("the library was called"), raising=True)


@pytest.mark.parametrize("bad", [np.zeros((4, 8), np.float32), np.zeros(4, np.float64), np.zeros((2, 2), SPHERE_DTYPE),
                                 (C.c_float * 8)(), [1.0, 2.0], "spheres", None, 3, [object()]],
                         ids=["f32 matrix", "f64", "2-d records", "ctypes floats", "floats", "str", "None", "int", "objects"])
def test_the_wrappers_refuse_a_wrong_dtype_or_shape(bad, no_library):
    with pytest.raises(ValueError):
        Context.set_spheres(_NoLibrary(), bad)
    with pytest.raises(ValueError):
        Node.set_spheres(_NoLibrary(), bad)


@pytest.mark.parametrize("count, ptr", [(-1, 0x1000), (2 ** 32, 0x1000), (1.5, 0x1000), ("2", 0x1000), (True, 0x1000), (1, -4), (1, 1.0), (1, None), (1, True)])
def test_set_spheres_device_refuses_a_count_that_is_no_u32_and_a_pointer_that_is_no_address(count, ptr, no_library):
    with pytest.raises(ValueError):
        Context.set_spheres_device(_NoLibrary(), count, ptr)


# ---- Layer.set_world / Raytracer.set_world ----

class _Target:
    """Stands for a Context / Node in set_world: records the calls, fails on demand."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], fail

    def set_spheres(self, spheres):
        self.calls.append(("set_spheres", len(spheres)))
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


def _new_world(k=4):
    return [m.Sphere((7 + i, 7, 7), 2.0, 2 - i % 3) for i in range(k)]


def test_layer_set_world_picks_set_spheres_or_set_scene_and_renders():
    layer, rp = _layer(None, False)                                 # nothing resident: only `world` changes
    layer.set_world(_new_world(), rp)
    assert len(layer.world) == 4 and layer.world[1].material_idx == 1 and layer._rgba is None
    t = _Target()
    layer, rp = _layer(t, True)                                     # an HBM scene: the sphere table alone
    layer.set_world(_new_world(9), rp)
    assert t.calls == [("set_spheres", 9), ("render", 8, 6, rp.sampling.num_samples_per_pixel)]
    assert len(layer.world) == 9 and layer.world[0].center.tolist() == [7.0, 7.0, 7.0] and layer._rgba.shape == (6, 8, 4) and layer._hbm is True
    t = _Target()
    layer, rp = _layer(t, False)                                    # an LDS scene: set again, with the new world
    layer.set_world(_new_world(2))
    assert t.calls == [("set_scene", 2, {})] and len(layer.world) == 2 and layer._hbm is False
    t = _Target()
    layer, rp = _layer(t, True)
    layer.set_world([])                                             # the empty world is a world
    assert t.calls == [("set_spheres", 0)] and layer.world == []
    with pytest.raises(ValueError):
        layer.set_world([m.Sphere((0, 0, 0), 1.0, 0).to_c()])
    assert t.calls == [("set_spheres", 0)]


def test_raytracer_set_world_picks_set_spheres_or_set_scene_and_restarts_the_accumulation():
    for hbm, want in ((True, [("set_spheres", 4)]), (False, [("set_scene", 4, {})])):
        rt = m.Raytracer.__new__(m.Raytracer)
        rt.spheres = [m.Sphere((i, 0, 0), 1.0, 0) for i in range(6)]
        rt.material_data, rt.global_texture_data, rt.sky_state = [], np.zeros((0, 3), np.float32), None
        rt.camera = m.GpuCamera.new(m.FlyCameraController.default().renderer_camera(), (8, 6))
        rt._ctx, rt._hbm, rt._accumulated = _Target(), hbm, 3
        rt.set_world(_new_world())
        assert rt._ctx.calls == want and len(rt.spheres) == 4 and rt._accumulated is None and rt._hbm is hbm


@pytest.mark.parametrize("status, keeps_hbm", [(_abi.MIRT_ERR_SCENE_TOO_LARGE, True), (_abi.MIRT_ERR_NULL_POINTER, True), (_abi.MIRT_ERR_HIP, False),
                                               (_abi.MIRT_ERR_ALLOC, False), (_abi.MIRT_ERR_NO_SCENE, False)])
def test_a_failed_set_world_leaves_the_held_world_alone(status, keeps_hbm):
    layer, rp = _layer(_Target(fail=status), True)
    with pytest.raises(m.MirtError):
        layer.set_world(_new_world(), rp)
    assert len(layer.world) == 6 and layer._rgba is None and layer._hbm is keeps_hbm    # after a lost scene the next call sets it again
    layer, rp = _layer(_Target(fail=status), False)
    with pytest.raises(m.MirtError):
        layer.set_world(_new_world())
    assert len(layer.world) == 6
    rt = m.Raytracer.__new__(m.Raytracer)
    rt.spheres = [m.Sphere((i, 0, 0), 1.0, 0) for i in range(6)]
    rt._ctx, rt._hbm, rt._accumulated = _Target(fail=status), True, 3
    with pytest.raises(m.MirtError):
        rt.set_world(_new_world())
    assert len(rt.spheres) == 6 and rt._hbm is keeps_hbm and rt._accumulated == 3


# ---- the inputs of tests/test_gpu_set_spheres.py's always-list cases exercise what they say ----

@pytest.mark.parametrize("name", list(ALWAYS_WORLDS))
def test_the_always_list_worlds_have_the_lists_they_claim(name):
    build, claimed = ALWAYS_WORLDS[name]
    arr = build()
    carr, keep = c_spheres(arr)
    rule = bvh_check.always_list(arr["center"][:, :3], arr["radius"])
    assert m.bvh_plan(carr)["n_always"] == len(rule) == claimed
    assert np.array_equal(build().view(np.uint8), arr.view(np.uint8))           # the same world every time it is asked for


def test_the_shared_cap_takes_the_tied_spheres_at_the_lowest_indices():
    arr, want = shared_cap_expected()
    assert np.array_equal(bvh_check.always_list(arr["center"][:, :3], arr["radius"]), want)
