"""Progressive frames in one launch (mirt_ctx_accum_frame_device / mirt_ctx_accum_frame, mirt_node_accum_*): every check is exact --
bytes of images, integers of sums and counts.  A fused frame must equal mirt_ctx_accum_add + mirt_ctx_accum_resolve on a second
context fed the same sequence, and one launch of the total sample count; a node's frame must equal a single context's."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from hbm_worlds import look, rtiow_field, scene_from_arrays
from helpers import assert_images_equal, scene_data

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DEMO = ROOT / "weekend-raytracer-wgpu_amd" / "host" / "layer_demo"
SEQUENCE = (2, 2, 5, 16, 32, 1, 64)           # lane-per-pixel, its streaming build and the pooled kernel all occur
LINEAR = m.MIRT_FLAG_NO_TONEMAP | m.MIRT_FLAG_NO_SRGB


def _pt(w, h, spp, **kw):
    kw.setdefault("num_bounces", 8)
    kw.setdefault("mode", m.MIRT_MODE_PT)
    return m.make_params(w, h, spp, **kw)


def _sky_blob():
    sky = _abi.MirtSkyState()
    for c in range(3):
        for i, v in enumerate((-1.1, -0.3, 0.8, 1.7, -2.0, 0.4, 0.2, 1.5, 0.6)):
            sky.params[9 * c + i] = v * (1.0 + 0.1 * c)
        sky.radiances[c] = 1.0 + c
    sky.sun_direction[:] = [0.0, 0.6, 0.8, 0.0]
    return sky


@pytest.fixture(scope="module")
def ctxs():
    """Three contexts: the fused frame into device memory, the fused frame into host memory, and add + resolve."""
    cs = [m.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def _device_frame(ctx, params, stream=None):
    """One fused frame into a fresh device buffer -> its bytes (after the context has drained)."""
    import torch
    out = torch.zeros((m.params_out_rows(params), params.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.accum_frame_device(params, out.data_ptr(), stream)
    ctx.synchronize()
    return out.cpu().numpy()


def _run_sequence(ctxs, sd, mk, what, *, hbm=False, sequence=SEQUENCE, one_launch=True, images=True):
    """The sequence on the three contexts; after EVERY frame: device image == host image == add + resolve, sums equal, image ==
    one launch of the total.  Returns the kernels the fused context ran, its final image and sums."""
    fused, host, two = ctxs
    for c in ctxs:
        c.set_scene(sd, hbm=hbm)
        c.accum_reset(mk(sequence[0]))
    kernels, total, img, sums = [], 0, None, None
    for k, spp in enumerate(sequence):
        p = mk(spp)
        img = _device_frame(fused, p)
        kernels.append(fused.last_kernel())
        img_host = host.accum_frame(p)
        two.accum_add(p)
        assert "_frame_kernel" in kernels[-1], kernels[-1]
        assert two.last_kernel() == kernels[-1].replace("_frame_kernel", "_kernel"), (two.last_kernel(), kernels[-1])    # the schedule of accum_add
        total += spp
        assert fused.accum_samples() == host.accum_samples() == two.accum_samples() == total
        sums = fused.accum_read(p)
        assert np.array_equal(sums, two.accum_read(p)), f"{what}: sums after frame {k} ({spp} spp)"
        assert np.array_equal(sums, host.accum_read(p)), f"{what}: host-form sums after frame {k}"
        if images:
            assert_images_equal(img, two.accum_resolve(p), f"{what}: frame {k} ({spp} spp) against add + resolve")
            assert_images_equal(img_host, img, f"{what}: frame {k} host form against device form")
            if one_launch:
                assert_images_equal(img, two.render(mk(total)), f"{what}: frame {k} against one launch of {total} spp")
    return kernels, img, sums


def test_fused_equals_two_step_three_spheres(ctxs, oracle):
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    mk = lambda spp: _pt(w, h, spp, seed=3)                                     # noqa: E731
    kernels, img, sums = _run_sequence(ctxs, sd, mk, "three spheres")
    assert len(set(kernels)) >= 3, kernels
    assert any(k.startswith("render_pt_strip_frame_kernel<") for k in kernels), kernels
    assert any(k.startswith("render_pt_stream_frame_kernel<") for k in kernels), kernels
    assert any(k.startswith("render_pt_pool_frame_kernel<") for k in kernels), kernels
    # against the oracle at the total sample count: every pixel's sums, then the image
    total = sum(SEQUENCE)
    want = oracle.render_pt_sums(sd, mk(total))
    assert np.array_equal(sums, want), f"{int((sums != want).any(-1).sum())} of {w * h} pixels differ from the oracle"
    assert_images_equal(img, oracle.render(sd, mk(total)), "final frame against the oracle")


@pytest.mark.parametrize("tiles", [False, True])
def test_fused_equals_two_step_main_rs_scene_with_image_textures(ctxs, tiles):
    w, h = 256, 144
    sd = scene_data("main_rs_scene", w, h)
    flags = m.MIRT_FLAG_TEXEL_TILES if tiles else 0
    kernels, _, _ = _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, flags=flags), f"main.rs scene tiles={tiles}")
    pool = "render_pt_pool_tile_frame_kernel<" if tiles else "render_pt_pool_frame_kernel<"
    assert kernels[4].startswith(pool) and kernels[6].startswith(pool), kernels           # 32 and 64 spp


def test_fused_equals_two_step_rtiow_grid_builds(ctxs):
    w, h = 192, 108
    sd = scene_data("rtiow_final", w, h)
    kernels, _, _ = _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, seed=1), "RTIOW")
    assert kernels[0] == "render_pt_strip_frame_kernel<false,false,true,true>", kernels                # the strip kernel's grid build
    grid_pool = [k for k in kernels if k.startswith("render_pt_pool_frame_kernel<") and (k.endswith(",true,true>") or k.endswith(",true,false>"))]
    assert grid_pool, kernels                                                                          # the pooled kernel's grid build


def test_fused_equals_two_step_hbm_world(ctxs):
    w, h = 160, 90
    arr, mats, tex = rtiow_field(6000, seed=6)
    sd = scene_from_arrays(look(w, h, (13, 2, 3), (0, 0, 0), vfov=30), arr, mats, tex)
    kernels, _, _ = _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp), "HBM world", hbm=True, sequence=(2, 2, 5, 16, 1))
    assert all(k.startswith("render_pt_hbm_frame_kernel<") for k in kernels), kernels
    for c in ctxs:                                     # leave no HBM scene behind on the shared contexts
        c.set_scene(scene_data("three_spheres", 64, 48))


@pytest.mark.parametrize("flags", [m.MIRT_FLAG_SKY_HOSEK, m.MIRT_FLAG_NO_TONEMAP, m.MIRT_FLAG_NO_SRGB, m.MIRT_FLAG_SKY_HOSEK | LINEAR])
def test_fused_equals_two_step_sky_and_tone_curve_flags(ctxs, flags):
    w, h = 200, 120
    sd = scene_data("three_spheres", w, h)
    sd.sky = _sky_blob()
    _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, flags=flags, seed=9), f"flags {flags:#x}")


def test_fused_equals_two_step_counting_launches(ctxs):
    """MIRT_FLAG_COUNT_WORK: the lane-per-sample strip kernel and its `my_px` hand-off."""
    w, h = 150, 70
    sd = scene_data("three_spheres", w, h)
    flags = m.MIRT_FLAG_COUNT_WORK | m.MIRT_FLAG_KERNEL_STRIP                  # (70 spp: two batches of 64 lanes; without the hint the pool's counting build)
    kernels, _, _ = _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, flags=flags), "counting", sequence=(2, 5, 70, 1))
    _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, flags=m.MIRT_FLAG_COUNT_WORK), "counting, default schedule", sequence=(2, 40))
    assert all(k.startswith("render_pt_strip_frame_kernel<true,false,false,false>") for k in kernels), kernels


def test_fused_equals_two_step_row_band_odd_width(ctxs):
    w, h = 317, 181
    sd = scene_data("three_spheres", w, h)
    mk = lambda spp: _pt(w, h, spp, seed=5, row_begin=37, row_end=150)          # noqa: E731
    _, img, _ = _run_sequence(ctxs, sd, mk, "band, odd width")
    assert img.shape == (113, w, 4)
    # ... and a part of a tile interleave (what a node's member runs)
    mk = lambda spp: _pt(w, h, spp, seed=5, row_begin=37, row_end=150, tile_rows=4, n_parts=3, part=1)   # noqa: E731
    _run_sequence(ctxs, sd, mk, "part 1/3 of the band", sequence=(2, 5, 32))


def test_fast_math_sums_equal_accum_add(ctxs):
    """MIRT_FLAG_FAST_MATH carries no image parity claim; the fused frame's SUMS equal accum_add's under the same flag."""
    w, h = 200, 120
    sd = scene_data("three_spheres", w, h)
    kernels, _, _ = _run_sequence(ctxs, sd, lambda spp: _pt(w, h, spp, flags=m.MIRT_FLAG_FAST_MATH), "fast math", images=False)
    assert all(k.startswith("fast_build::render_pt_") for k in kernels), kernels


def test_reference_render_loop_against_the_oracle(ctxs, oracle):
    """The reference's loop shape: main.rs's scene, 2 samples per pixel and frame seeded as Raytracer::render_frame seeds them
    (frame_spp = 2), 16 fused frames against ONE oracle pass over all 32: the sums of every pixel, then the image."""
    w, h, n, total = 480, 270, 2, 32
    sd = scene_data("main_rs_scene", w, h)
    ctx = ctxs[0]
    ctx.set_scene(sd)
    mk = lambda spp: _pt(w, h, spp, frame_spp=n)                                # noqa: E731
    ctx.accum_reset(mk(n))
    img = None
    for _ in range(total // n):
        img = _device_frame(ctx, mk(n))
    assert ctx.accum_samples() == total and ctx.last_kernel().startswith("render_pt_strip_frame_kernel<")
    got, want = ctx.accum_read(mk(n)), oracle.render_pt_sums(sd, mk(total))
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} of {w * h} pixels differ"
    assert_images_equal(img, oracle.render(sd, mk(total)), "the last fused frame")


def test_reference_stream_frames_and_a_refused_frame(ctxs):
    """frame_spp = 2, frame_begin = 7: eight fused 2-spp frames == one launch of 16 spp; a 3-spp frame in between is refused and
    changes nothing."""
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    ctx, _, other = ctxs
    ctx.set_scene(sd)
    other.set_scene(sd)
    mk = lambda spp: _pt(w, h, spp, seed=4, frame_spp=2, frame_begin=7)        # noqa: E731
    ctx.accum_reset(mk(2))
    img = None
    for k in range(8):
        if k == 3:
            before = ctx.accum_read(mk(2))
            with pytest.raises(m.MirtError) as e:
                ctx.accum_frame(mk(3))
            assert e.value.status == _abi.MIRT_ERR_FRAME_SPP
            import torch
            out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            with pytest.raises(m.MirtError) as e:
                ctx.accum_frame_device(mk(3), out.data_ptr())
            assert e.value.status == _abi.MIRT_ERR_FRAME_SPP
            assert ctx.accum_samples() == 6 and np.array_equal(ctx.accum_read(mk(2)), before)
        img = _device_frame(ctx, mk(2))
    assert ctx.accum_samples() == 16
    assert_images_equal(img, other.render(mk(16)), "eight 2-spp frames against one 16-spp launch")
    assert_images_equal(ctx.accum_frame(mk(0)), img, "spp == 0 with frame_spp set: the mean of what is there")
    assert ctx.accum_samples() == 16
    other.accum_reset(mk(16))
    other.accum_add(mk(16))
    assert np.array_equal(ctx.accum_read(mk(2)), other.accum_read(mk(16)))


def test_spp_zero_resolves_what_is_there(ctxs):
    import torch
    w, h = 200, 120
    sd = scene_data("three_spheres", w, h)
    ctx = ctxs[0]
    ctx.set_scene(sd)
    ctx.accum_reset(_pt(w, h, 2))
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    for call in (lambda: ctx.accum_frame(_pt(w, h, 0)), lambda: ctx.accum_frame_device(_pt(w, h, 0), out.data_ptr())):
        with pytest.raises(m.MirtError) as e:
            call()
        assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    for call in (lambda: ctx.accum_add(_pt(w, h, 0)), lambda: ctx.render(_pt(w, h, 0))):          # only the frame calls accept spp == 0
        with pytest.raises(m.MirtError) as e:
            call()
        assert e.value.status == _abi.MIRT_ERR_SPP_ZERO
    ctx.accum_frame(_pt(w, h, 6))
    sums = ctx.accum_read(_pt(w, h, 6))
    for flags in (0, LINEAR):
        want = ctx.accum_resolve(_pt(w, h, 6, flags=flags))
        assert_images_equal(_device_frame(ctx, _pt(w, h, 0, flags=flags)), want, "spp == 0, device form")
        assert ctx.last_kernel() == "resolve_accum_kernel"
        assert_images_equal(ctx.accum_frame(_pt(w, h, 0, flags=flags)), want, "spp == 0, host form")
        assert ctx.accum_samples() == 6 and np.array_equal(ctx.accum_read(_pt(w, h, 6)), sums)
    # output checks and a geometry other than the reset's
    with pytest.raises(m.MirtError) as e:
        ctx.accum_frame_device(_pt(w, h, 2), out.data_ptr(), None, nbytes=out.numel() - 4)
    assert e.value.status == _abi.MIRT_ERR_OUT_BUFFER
    with pytest.raises(m.MirtError) as e:
        ctx.accum_frame_device(_pt(w, h, 2), 0)
    assert e.value.status == _abi.MIRT_ERR_NULL_POINTER
    with pytest.raises(m.MirtError) as e:
        ctx.accum_frame(_pt(w, h - 1, 2))
    assert e.value.status == _abi.MIRT_ERR_OUT_BUFFER
    assert ctx.accum_samples() == 6 and np.array_equal(ctx.accum_read(_pt(w, h, 6)), sums)


def test_two_frames_in_flight_and_resolve_after_a_caller_stream(ctxs):
    """Fused frames alternate on the context's two frame streams into two device buffers; each buffer is read back after ITS
    stream's sync only.  Every frame equals the serial sequence.  Then one frame on a caller stream followed by
    mirt_ctx_accum_resolve with no sync in between."""
    import torch
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    seq = (2, 2, 5, 16, 32, 1, 64, 2, 2, 2, 2, 2)
    ctx, _, serial = ctxs
    mk = lambda spp: _pt(w, h, spp, seed=8)                                     # noqa: E731
    serial.set_scene(sd)
    serial.accum_reset(mk(2))
    wants = [serial.accum_frame(mk(spp)) for spp in seq]
    ctx.set_scene(sd)
    ctx.accum_reset(mk(2))
    streams = [ctx.frame_stream(0), ctx.frame_stream(1)]
    waits = [torch.cuda.ExternalStream(s) for s in streams]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k, spp in enumerate(seq):
        if k >= 2:                                     # framebuffer k & 1 still holds frame k - 2: wait for its stream, read it
            waits[k & 1].synchronize()
            assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k - 2], f"frame {k - 2} of two in flight")
        ctx.accum_frame_device(mk(spp), bufs[k & 1].data_ptr(), streams[k & 1])
    for k in (len(seq) - 2, len(seq) - 1):
        waits[k & 1].synchronize()
        assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k], f"frame {k} of two in flight")
    assert ctx.accum_samples() == sum(seq)
    assert np.array_equal(ctx.accum_read(mk(2)), serial.accum_read(mk(2)))
    # a caller stream, then resolve at once
    side = torch.cuda.Stream()
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.accum_frame_device(mk(16), out.data_ptr(), side.cuda_stream)
    resolved = ctx.accum_resolve(mk(16))
    want = serial.accum_frame(mk(16))
    assert_images_equal(resolved, want, "accum_resolve right after a frame on a caller stream")
    side.synchronize()
    assert_images_equal(out.cpu().numpy(), want, "the frame on the caller stream")


def test_frames_that_only_read_take_part_in_the_ordering(ctxs):
    """Frames of 2, 0, 2, 0, ... spp alternating on the two frame streams into two buffers (a host that presents every vsync and
    adds every other frame): the adding frame must not rewrite sums the spp == 0 frame on the other stream is still reading.
    The reading frame's stream is kept busy in front of it (a few milliseconds of matrix products), so the read is still PENDING when
    the next adding frame is queued: without the ordering that frame runs first and the read shows new sums over the old count.
    Then spp == 0 frames on two caller streams, the first behind such a load, followed AT ONCE by accum_reset and a frame: the
    reset must wait for both reads."""
    import torch
    ballast = torch.rand((4096, 4096), device="cuda")

    def keep_busy(stream):
        with torch.cuda.stream(stream):
            for _ in range(6):
                torch.mm(ballast, ballast)
    w, h = 1920, 1080
    sd = scene_data("three_spheres", w, h)
    ctx, _, serial = ctxs
    mk = lambda spp: _pt(w, h, spp, seed=12)                                    # noqa: E731
    seq = (2, 0) * 8
    serial.set_scene(sd)
    serial.accum_reset(mk(2))
    wants = [serial.accum_frame(mk(spp)) for spp in seq]
    for k in range(1, len(seq), 2):
        assert np.array_equal(wants[k], wants[k - 1])                           # (a frame that adds nothing shows what the last one showed)
    ctx.set_scene(sd)
    ctx.accum_reset(mk(2))
    streams = [ctx.frame_stream(0), ctx.frame_stream(1)]
    waits = [torch.cuda.ExternalStream(s) for s in streams]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k, spp in enumerate(seq):                      # the adding frames on stream 0, the reading ones on stream 1
        if k >= 2:
            waits[k & 1].synchronize()
            assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k - 2], f"frame {k - 2} ({seq[k - 2]} spp) of 2, 0, 2, 0, ...")
        if spp == 0:
            keep_busy(waits[1])
        ctx.accum_frame_device(mk(spp), bufs[k & 1].data_ptr(), streams[k & 1])
    for k in (len(seq) - 2, len(seq) - 1):
        waits[k & 1].synchronize()
        assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k], f"frame {k} of 2, 0, 2, 0, ...")
    assert ctx.accum_samples() == sum(seq) and np.array_equal(ctx.accum_read(mk(2)), serial.accum_read(mk(2)))
    # two reading frames on two caller streams, then reset + a frame with no sync in between
    side = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for rounds in range(3):
        keep_busy(side[0])
        ctx.accum_frame_device(mk(0), outs[0].data_ptr(), side[0].cuda_stream)
        ctx.accum_frame_device(mk(0), outs[1].data_ptr(), side[1].cuda_stream)
        ctx.accum_reset(mk(2))
        ctx.accum_frame_device(mk(2), outs[2].data_ptr(), side[0].cuda_stream)
        side[0].synchronize()
        side[1].synchronize()
        want_before = wants[-1] if rounds == 0 else wants[0]
        assert_images_equal(outs[0].cpu().numpy(), want_before, f"round {rounds}: the read on caller stream 0 before the reset")
        assert_images_equal(outs[1].cpu().numpy(), want_before, f"round {rounds}: the read on caller stream 1 before the reset")
        assert_images_equal(outs[2].cpu().numpy(), wants[0], f"round {rounds}: the first frame after the reset")
        assert ctx.accum_samples() == 2


# ---- node ----

NODE_SEQUENCE = (2, 2, 5, 16, 32, 1, 0)


def _single_context_frames(ctx, sd, mk, sequence=NODE_SEQUENCE):
    ctx.set_scene(sd)
    ctx.accum_reset(mk(2))
    out = []
    for spp in sequence:
        img = _device_frame(ctx, mk(spp))
        out.append((img, ctx.accum_read(mk(2)), ctx.accum_samples()))
    return out


def _check_node(node, sd, mk, wants, what, sequence=NODE_SEQUENCE):
    node.set_scene(sd)
    node.accum_reset(mk(2))
    assert node.accum_samples() == 0
    for k, (spp, (img, sums, count)) in enumerate(zip(sequence, wants)):
        assert_images_equal(node.accum_frame(mk(spp)), img, f"{what}: frame {k} ({spp} spp)")
        assert np.array_equal(node.accum_read(mk(2)), sums), f"{what}: sums after frame {k}"
        assert node.accum_samples() == count


def test_node_frames_match_one_context(ctxs):
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    mk = lambda spp: _pt(w, h, spp, seed=6)                                     # noqa: E731
    wants = _single_context_frames(ctxs[0], sd, mk)
    for n in (1, 2, 4, 8):
        with m.Node([0] * n) as node:
            _check_node(node, sd, mk, wants, f"loopback N={n}")
            st = node.stats()
            assert (st["n_members"], st["transport"]) == (n, 0), st
            if n > 1:
                assert node.context(n - 1).last_kernel() == "resolve_accum_kernel"        # the spp == 0 frame ran on every member
    with m.Node([0], rccl=True) as node:
        _check_node(node, sd, mk, wants, "forced RCCL")
        st = node.stats()
        assert (st["n_members"], st["transport"]) == (1, 1) and st["assemble_ms"] > 0.0, st


def test_node_frame_into_device_memory_on_a_caller_stream(ctxs):
    import torch
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    mk = lambda spp: _pt(w, h, spp, seed=6)                                     # noqa: E731
    seq = (2, 2, 5, 16)
    wants = _single_context_frames(ctxs[0], sd, mk, seq)
    side = torch.cuda.Stream()
    outs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in seq]
    torch.cuda.synchronize()
    with m.Node([0] * 4) as node:
        node.set_scene(sd)
        node.accum_reset(mk(2))
        for spp, out in zip(seq, outs):                # queued back to back, no host sync in between
            node.accum_frame_device(mk(spp), out.data_ptr(), side.cuda_stream)
        side.synchronize()
        for k, (out, (img, _, _)) in enumerate(zip(outs, wants)):
            assert_images_equal(out.cpu().numpy(), img, f"queued node frame {k}")
        assert np.array_equal(node.accum_read(mk(2)), wants[-1][1]) and node.accum_samples() == wants[-1][2]


def test_node_members_without_rows_and_odd_width(ctxs):
    for (w, h, n, kw) in ((64, 8, 8, {}), (318, 101, 3, {}), (317, 181, 4, dict(row_begin=37, row_end=150))):
        sd = scene_data("three_spheres", w, h)
        mk = lambda spp: _pt(w, h, spp, seed=2, **kw)                           # noqa: E731
        wants = _single_context_frames(ctxs[0], sd, mk)
        with m.Node([0] * n) as node:
            _check_node(node, sd, mk, wants, f"{w}x{h} N={n}")
            if h == 8:                                 # tiles of 4 rows: members 2..7 have no rows and ran nothing
                assert [node.context(i).last_kernel() != "" for i in range(8)] == [True, True] + [False] * 6


def test_node_refusals_and_invalidation(ctxs):
    import torch
    w, h = 320, 182
    sd = scene_data("three_spheres", w, h)
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")

    def refused(call, status):
        with pytest.raises(m.MirtError) as e:
            call()
        assert e.value.status == status, (e.value.status, status)

    with m.Node([0] * 4) as node:
        refused(lambda: node.accum_reset(_pt(w, h, 2)), _abi.MIRT_ERR_NO_SCENE)
        node.set_scene(sd)
        refused(lambda: node.accum_frame(_pt(w, h, 2)), _abi.MIRT_ERR_OUT_BUFFER)                    # before the reset
        assert "mirt_node_accum_reset" in m.lib().mirt_last_error().decode()
        refused(lambda: node.accum_reset(_pt(w, h, 2, tile_rows=4, n_parts=2)), _abi.MIRT_ERR_BAD_ROWS)
        node.accum_reset(_pt(w, h, 2))
        refused(lambda: node.accum_frame(_pt(w, h, 0)), _abi.MIRT_ERR_NO_SCENE)                      # nothing accumulated yet
        refused(lambda: node.accum_frame(_pt(w, h, 2, tile_rows=4, n_parts=4, part=1)), _abi.MIRT_ERR_BAD_ROWS)
        refused(lambda: node.accum_frame(_pt(w, h - 2, 2)), _abi.MIRT_ERR_OUT_BUFFER)                # another geometry
        refused(lambda: node.accum_frame(_pt(w, h, 2, row_begin=4)), _abi.MIRT_ERR_OUT_BUFFER)
        refused(lambda: node.accum_frame_device(_pt(w, h, 2), out.data_ptr(), 0), _abi.MIRT_ERR_HIP)   # hipStreamLegacy
        refused(lambda: node.accum_frame(_pt(w, h, 3, frame_spp=2)), _abi.MIRT_ERR_FRAME_SPP)
        assert node.accum_samples() == 0
        node.accum_frame(_pt(w, h, 2))                 # none of the refusals has invalidated the accumulation
        assert node.accum_samples() == 2
        # what a member refuses before it queues anything (here: Hosek sky without a sky blob) is found by asking every member
        # first, by the context's own rules: nothing was queued, the accumulation stays valid
        refused(lambda: node.accum_frame(_pt(w, h, 2, flags=m.MIRT_FLAG_SKY_HOSEK)), _abi.MIRT_ERR_SKY)
        refused(lambda: node.accum_frame_device(_pt(w, h, 2, flags=m.MIRT_FLAG_SKY_HOSEK), out.data_ptr()), _abi.MIRT_ERR_SKY)
        assert node.accum_samples() == 2
        node.accum_frame(_pt(w, h, 2))
        assert node.accum_samples() == 4
        # set_scene / set_camera do not touch the sums; the host resets
        node.accum_reset(_pt(w, h, 2))
        node.accum_frame(_pt(w, h, 2))
        node.set_scene(sd)
        node.set_camera(sd.camera)
        assert node.accum_samples() == 2
        ctx = ctxs[0]
        ctx.set_scene(sd)
        ctx.accum_reset(_pt(w, h, 2))
        ctx.accum_frame(_pt(w, h, 2))
        assert_images_equal(node.accum_frame(_pt(w, h, 2)), ctx.accum_frame(_pt(w, h, 2)), "after set_scene / set_camera")


def test_raytracer_on_a_node_equals_raytracer_on_a_context():
    """Ten render_frame calls across a set_render_params reset, past max_samples_per_pixel (the spp == 0 frames)."""
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(160, 90), sampling=m.SamplingParams(8, 2, 8))
    frames = []
    for kw in (dict(device=0), dict(devices=[0, 0, 0])):
        rt = m.Raytracer(scene, rp, **kw)
        imgs = []
        for k in range(10):
            if k == 6:
                rt.set_render_params(rp)
            imgs.append(rt.render_frame())
        assert rt.progress() == 1.0 and rt.frame_number == 11
        frames.append(imgs)
        rt.close()
    for k, (a, b) in enumerate(zip(*frames)):
        assert_images_equal(b, a, f"render_frame call {k}: node against context")
    assert not np.array_equal(frames[0][0], frames[0][3])          # the loop did progress ...
    assert np.array_equal(frames[0][3], frames[0][5])              # ... and stopped adding at max_samples_per_pixel


def test_raytracer_render_frame_device_keeps_two_frames_in_flight():
    import torch
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(160, 90), sampling=m.SamplingParams(8, 2, 8))
    rt = m.Raytracer(scene, rp)
    wants = [rt.render_frame() for _ in range(6)]
    rt.set_render_params(rp)
    bufs = [torch.zeros((90, 160, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    used = []
    for k in range(6):
        if k >= 2:
            torch.cuda.ExternalStream(used[k - 2]).synchronize()
            assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k - 2], f"frame {k - 2}")
        used.append(rt.render_frame_device(bufs[k & 1].data_ptr()))
    assert used[0] != used[1] and used[0] == used[2]
    for k in (4, 5):
        torch.cuda.ExternalStream(used[k]).synchronize()
        assert_images_equal(bufs[k & 1].cpu().numpy(), wants[k], f"frame {k}")
    rt.close()


def test_raytracer_render_frame_device_on_a_node_needs_a_stream():
    import torch
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(160, 90), sampling=m.SamplingParams(8, 2, 8))
    rt = m.Raytracer(scene, rp)
    wants = [rt.render_frame() for _ in range(5)]
    rt.close()
    rt = m.Raytracer(scene, rp, devices=[0, 0])
    out = torch.zeros((90, 160, 4), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        rt.render_frame_device(out.data_ptr())
    assert rt.frame_number == 1 and rt.progress() == 0.0          # the refused call issued nothing
    for k, want in enumerate(wants):
        assert rt.render_frame_device(out.data_ptr(), side.cuda_stream) == side.cuda_stream
        side.synchronize()
        assert_images_equal(out.cpu().numpy(), want, f"node frame {k} into device memory")
    rt.close()


def test_cpp_raytracer_on_a_node(tmp_path, oracle):
    """host/mirt_host.hpp: Raytracer on a device list -- 4 progressive frames of 4 spp of the main.rs scene through a 3-member
    node (mirt_node_accum_frame) until progress() is 1, then one more render_frame (layer_demo.cpp: "one more: must change
    nothing" -- the spp == 0 frame), whose image the demo writes: == 16 spp in one go."""
    ppm = {}
    for name in ("moon", "earthmap"):
        a = np.load(m.asset_path(f"assets/{name}.jpeg"))["rgb8"]
        ppm[name] = tmp_path / f"{name}.ppm"
        with open(ppm[name], "wb") as f:
            f.write(b"P6\n1024 512\n255\n")
            f.write(a.tobytes())
    subprocess.run(["make", "-C", str(DEMO.parent)], check=True, capture_output=True)
    out = tmp_path / "pt.rgba"
    w, h = 96, 54
    r = subprocess.run([str(DEMO), "--pt", str(ppm["moon"]), str(ppm["earthmap"]), str(w), str(h), "4", "16", str(out), "0,0,0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.startswith("pt: 4 frames, progress 1.00")
    got = np.fromfile(out, dtype=np.uint8).reshape(h, w, 4)
    want = oracle.render(scene_data("main_rs_scene", w, h), _pt(w, h, 16))
    assert_images_equal(got, want, "C++ Raytracer on a node")
