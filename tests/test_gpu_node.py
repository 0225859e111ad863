"""The node (mirt_node_*): one process cuts a frame across member contexts and assembles it on member 0.  Every image is
compared byte for byte with mirt_ctx_render of the same params on a plain context.  One GPU: loopback nodes (every member on
device 0) and the forced one-rank RCCL node."""
import ctypes as C

import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from helpers import assert_images_equal, scene_data

pytestmark = pytest.mark.gpu


def _pt(w, h, spp, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, num_bounces=8, **kw)


def _want(ctx, sd, params):
    ctx.set_scene(sd)
    return ctx.render(params)


def test_loopback_matches_one_context(gpu_ctx):
    """Config 3's three spheres at 320 x 182 (182 is no multiple of 4 N), path traced, five seeds, N = 2, 3, 4, 8."""
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    wants = {seed: _want(gpu_ctx, sd, _pt(w, h, 16, seed=seed)) for seed in range(5)}
    for n in (2, 3, 4, 8):
        with m.Node([0] * n) as node:
            node.set_scene(sd)
            for seed, want in wants.items():
                assert_images_equal(node.render(_pt(w, h, 16, seed=seed)), want, f"loopback N={n} seed={seed}")


def test_layer_set_data_through_a_node():
    """Parity mode: `Layer::scene` at 800 x 600, 2 spp, Layer(devices=[0] * 4).set_data against Layer().set_data."""
    rp = m.RenderParams(camera=m.FlyCameraController.default().renderer_camera(), viewport_size=(800, 600))
    images = []
    for devices in (None, [0] * 4):
        layer = m.Layer.new([800, 600], rp, devices=devices)
        assert layer.set_global_data()
        layer.set_data(rp)
        images.append(layer.register_texture().copy())
        if devices is not None:
            assert layer.last_stats["n_members"] == 4 and layer.last_stats["transport"] == 0
        layer.close()
    assert images[0].shape == (600, 800, 4)
    assert_images_equal(images[1], images[0], "Layer.set_data through a 4-member node")


def test_row_band_sample_offset_and_frame_spp(gpu_ctx):
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    p = _pt(w, h, 8, seed=7, row_begin=37, row_end=150, sample_begin=4, frame_spp=2, frame_begin=3)
    want = _want(gpu_ctx, sd, p)
    assert want.shape == (113, w, 4)
    for n in (3, 4):
        with m.Node([0] * n) as node:
            node.set_scene(sd)
            assert_images_equal(node.render(p), want, f"band N={n}")


def test_rtiow_4k_on_eight_members(gpu_ctx):
    """Config 5's scene (grid kernels on every member) at 3840 x 2160, 16 spp, N = 8."""
    w, h = 3840, 2160
    sd = scene_data("rtiow_final", w, h)
    p = _pt(w, h, 16, seed=3)
    want = _want(gpu_ctx, sd, p)
    with m.Node([0] * 8) as node:
        node.set_scene(sd)
        assert_images_equal(node.render(p), want, "RTIOW 4K N=8")
        for i in range(8):
            assert node.context(i).last_kernel().startswith("render_pt_"), i


def test_members_without_rows_are_skipped(gpu_ctx):
    """An 8-row frame on 8 members: tiles of 4 rows, so members 2..7 have no rows."""
    w, h = 64, 8
    sd = scene_data("three_spheres", w, h)
    p = _pt(w, h, 32, seed=1)
    want = _want(gpu_ctx, sd, p)
    with m.Node([0] * 8) as node:
        node.set_scene(sd)
        assert_images_equal(node.render(p), want, "8 rows, N=8")
        assert [node.context(i).last_kernel() != "" for i in range(8)] == [True, True] + [False] * 6


def test_odd_width_takes_the_dword_path(gpu_ctx):
    """Width 318 (rows not 16-byte aligned): through a loopback node, and through mirt_ctx_deinterleave_device (stride form)."""
    import torch
    w, h, spp = 318, 101, 12
    sd = scene_data("three_spheres", w, h)
    base = _pt(w, h, spp, seed=5)
    want = _want(gpu_ctx, sd, base)
    with m.Node([0] * 3) as node:
        node.set_scene(sd)
        assert_images_equal(node.render(base), want, "width 318, node N=3")
    world, tr = 4, 4
    max_rows = m.multi_gpu.max_part_rows(base, world, tr)
    parts = torch.zeros((world, max_rows, w, 4), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for r in range(world):
        pr = m.multi_gpu.part_params(base, r, world, tr)
        gpu_ctx.render_device(pr, parts[r].data_ptr(), m.params_out_rows(pr) * w * 4, stream)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    gpu_ctx.deinterleave_device(m.multi_gpu.part_params(base, 0, world, tr), parts.data_ptr(), max_rows * w * 4,
                                out.data_ptr(), out.numel(), stream)
    torch.cuda.synchronize()
    assert_images_equal(out.cpu().numpy(), want, "width 318, device de-interleave")


def test_forced_rccl_on_one_device(gpu_ctx):
    """devices = {0} with MIRT_NODE_RCCL: one real RCCL communicator (librccl through dlopen), the gather, the assembly.
    Created, used and destroyed twice in a row: the communicator is torn down."""
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    p = _pt(w, h, 16, seed=11)
    want = _want(gpu_ctx, sd, p)
    for attempt in range(2):
        with m.Node([0], rccl=True) as node:
            node.set_scene(sd)
            assert_images_equal(node.render(p), want, f"forced RCCL, node {attempt}")
            st = node.stats()
            assert (st["n_members"], st["transport"]) == (1, 1), st
            assert st["gather_ms"] >= 0.0 and st["assemble_ms"] > 0.0, st


def test_frames_queued_back_to_back_on_one_stream(gpu_ctx):
    """Five frames with different seeds through mirt_node_render_device into five device buffers on one caller stream, no host
    sync between them: each equals its own single-context render (members must not overwrite parts still being read)."""
    import torch
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    seeds = (21, 22, 23, 24, 25)
    wants = [_want(gpu_ctx, sd, _pt(w, h, 16, seed=s)) for s in seeds]
    side = torch.cuda.Stream()
    outs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in seeds]
    torch.cuda.synchronize()
    with m.Node([0] * 4) as node:
        node.set_scene(sd)
        for s, out in zip(seeds, outs):
            node.render_device(_pt(w, h, 16, seed=s), out.data_ptr(), out.numel(), side.cuda_stream)
        side.synchronize()
        for s, out, want in zip(seeds, outs, wants):
            assert_images_equal(out.cpu().numpy(), want, f"queued frame seed={s}")


def test_stats_contexts_and_refusals(gpu_ctx):
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    with m.Node([0] * 4) as node:
        with pytest.raises(m.MirtError) as e:
            node.render(_pt(w, h, 4))
        assert e.value.status == _abi.MIRT_ERR_NO_SCENE
        node.set_scene(sd)
        with pytest.raises(m.MirtError) as e:
            node.render(_pt(w, h, 4, tile_rows=4, n_parts=2))
        assert e.value.status == _abi.MIRT_ERR_BAD_ROWS
        node.render(_pt(w, h, 4))
        st = node.stats()
        assert (st["n_members"], st["transport"], st["gather_ms"]) == (4, 0, 0.0) and st["assemble_ms"] > 0.0, st
        for i in range(4):
            assert node.context(i).last_kernel().startswith("render_pt_"), i
        with pytest.raises(m.MirtError) as e:
            node.context(4)
        assert e.value.status == _abi.MIRT_ERR_BAD_ROWS
        # the default stream is refused (the node records and waits on events of the streams it is given)
        import torch
        out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(m.MirtError) as e:
            node.render_device(_pt(w, h, 4), out.data_ptr(), out.numel(), 0)
        assert e.value.status == _abi.MIRT_ERR_HIP
        # a failed set_scene leaves the node without a scene
        bad = sd.as_c()
        bad.camera = None
        assert m.lib().mirt_node_set_scene(node._h, C.byref(bad)) == _abi.MIRT_ERR_NULL_POINTER
        with pytest.raises(m.MirtError) as e:
            node.render(_pt(w, h, 4))
        assert e.value.status == _abi.MIRT_ERR_NO_SCENE
        node.set_scene(sd)
        assert_images_equal(node.render(_pt(w, h, 4, seed=2)), _want(gpu_ctx, sd, _pt(w, h, 4, seed=2)), "after a new set_scene")
