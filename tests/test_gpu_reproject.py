"""mirt_ctx_reproject* on the device against tests/reproject_ref.py: every comparison is every float32 record bit for bit (a NaN equal
to any NaN) AND every RGBA8 byte.  The colours come from real progressive frames through mirt_ctx_denoise (itself held to
tests/denoise_ref.py by test_gpu_denoise.py), the guides from mirt_ctx_render_features, or both are crafted by hand, so the
reprojection is the only thing under test.  One context for the module; a reference is computed once per (frames, parameters)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import FEATURE_DTYPE
import denoise_ref as dr
import feature_ref as fr
import hbm_worlds
import ray_query_ref as rq
import reproject_ref as rr

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = rr.MISS
LINEAR = m.MIRT_FLAG_NO_TONEMAP | m.MIRT_FLAG_NO_SRGB
W, H = fr.W, fr.H
EYE, AT = (13, 2, 3), (0, 0.5, 0)


def _look(w, h, eye=EYE, at=AT):
    return hbm_worlds.look(w, h, eye, at, vfov=25, aperture=0.0)


def second_cameras(w=W, h=H):
    """The camera of the CURRENT frame for a previous frame taken with _look(w, h): moved a little, moved a lot, turned by 180 degrees
    (it looks away from where the previous one looked), and equal to it."""
    away = tuple(2 * e - a for e, a in zip(EYE, AT))
    return {"moved a little": _look(w, h, (12.8, 2.1, 3.3)), "moved a lot": _look(w, h, (9.0, 4.0, 8.0)), "turned by 180 degrees": _look(w, h, EYE, away),
            "equal": _look(w, h)}


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _pt(w=W, h=H, spp=2, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, **kw)


def _same(got, want, what):
    (gf, gr), (wf, wr) = got, want
    assert gf.shape == wf.shape and gf.dtype == f32 and gr.shape == wr.shape and gr.dtype == np.uint8, what
    bad = np.argwhere(~rr.same_f32_or_nan(gf, wf).all(-1))
    bad8 = np.argwhere((gr != wr).any(-1))
    print(f"{what}: {wf.shape[0] * wf.shape[1]} pixels, {len(bad)} float32 records and {len(bad8)} RGBA8 pixels differ")
    assert len(bad) == 0, f"{what}: float32 differs at {bad[0]}: got {gf[tuple(bad[0])]}, want {wf[tuple(bad[0])]}"
    assert len(bad8) == 0, f"{what}: RGBA8 differs at {bad8[0]}: got {gr[tuple(bad8[0])]}, want {wr[tuple(bad8[0])]}"


def _frame(ctx, cam, p, seed):
    """One fresh frame of p.spp samples under `seed` with camera `cam` -> (the denoised colour float32 [rows, w, 4], its guides)."""
    ctx.set_camera(cam)
    q = _pt(p.width, p.height, p.spp, seed=seed, row_begin=p.row_begin, row_end=p.row_end)
    ctx.accum_reset(q)
    ctx.accum_frame(q)
    guides = ctx.render_features(q)
    colour = ctx.denoise(q, m.make_denoise_params("accum", levels=3, f32=True), guides)
    return colour, guides


def _with_lengths(colour, seed):
    """A denoise output as a history: its fourth channel, 1.0 everywhere, takes lengths from 1 to 9."""
    out = colour.copy()
    out[..., 3] = np.random.default_rng(seed).integers(1, 10, out.shape[:2]).astype(f32)
    return out


# ---- 1. the fixture frames: 67 x 45, neither a multiple of a tile nor of a wave ----

@pytest.fixture(scope="module")
def fixture_frames(ctx):
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt()
    prev_colour, prev_guides = _frame(ctx, _look(W, H), p, 0)
    prev_colour = _with_lengths(prev_colour, 1)
    cur = {}
    for i, (name, cam) in enumerate(second_cameras().items()):
        cur[name] = _frame(ctx, cam, p, 10 + i) + (cam,)
    assert (prev_guides["sphere"] == MISS).sum() > 500 and (prev_guides["sphere"] != MISS).sum() > 1000
    for a in (prev_colour, prev_guides) + tuple(x for v in cur.values() for x in v[:2]):
        a.setflags(write=False)
    ctx.set_camera(_look(W, H))
    return p, prev_colour, prev_guides, _look(W, H), cur


_references = {}


def _fixture_reference(frames, name, clamp, mh, dt, flags):
    key = (name, clamp, mh, dt, flags)
    if key not in _references:
        _, prev_colour, prev_guides, prev_cam, cur = frames
        colour, guides, cam = cur[name]
        _references[key] = rr.reproject(colour, guides, prev_colour, prev_guides, prev_cam, cam, W, H, max_history=mh, depth_tolerance=dt, clamp=clamp, flags=flags)
    return _references[key]


def test_the_small_move_finds_history_for_most_pixels_and_none_for_some(fixture_frames):
    """On the reference's own output: the comparison below is not one of frames without history, nor of frames with nothing else."""
    out = _fixture_reference(fixture_frames, "moved a little", True, 8.0, 0.05, 0)[0]
    have = rr.history_fraction(out)
    print(f"moved a little: history for {100 * have:.1f} % of the pixels")
    assert 0.5 <= have <= 0.99
    assert rr.history_fraction(_fixture_reference(fixture_frames, "equal", True, 8.0, 0.05, 0)[0]) > 0.9
    assert rr.history_fraction(_fixture_reference(fixture_frames, "turned by 180 degrees", True, 8.0, 0.05, 0)[0]) == 0.0
    assert 0.0 < rr.history_fraction(_fixture_reference(fixture_frames, "moved a lot", True, 8.0, 0.2, 0)[0]) < have


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "no clamp"])
@pytest.mark.parametrize("name", ["moved a little", "moved a lot", "turned by 180 degrees", "equal"])
def test_the_fixture_frames_match_the_reference(ctx, fixture_frames, name, clamp):
    p, prev_colour, prev_guides, prev_cam, cur = fixture_frames
    colour, guides, cam = cur[name]
    for mh in (1.0, 8.0, 2.0 ** 20):
        for dt in (0.0, 0.05):
            for flags in (0, LINEAR):
                r = m.make_reproject_params(prev_cam, cam, max_history=mh, depth_tolerance=dt, clamp=clamp)
                got = ctx.reproject(_pt(flags=flags), r, colour, guides, prev_colour, prev_guides, rgba8=True)
                assert ctx.last_kernel() == f"reproject_kernel<{'true' if clamp else 'false'},true>"
                _same(got, _fixture_reference(fixture_frames, name, clamp, mh, dt, flags), f"{name}, clamp {clamp}, max_history {mh}, depth_tolerance {dt}, flags {flags}")
    assert ctx.trace_stats()["kernel_ms"] > 0.0
    lin = ctx.reproject(p, r, colour, guides, prev_colour, prev_guides)           # without the RGBA8 plane: the other instantiation
    assert ctx.last_kernel() == f"reproject_kernel<{'true' if clamp else 'false'},false>"
    assert rr.same_f32_or_nan(lin, got[0]).all()
    if name == "moved a little":
        a, b = _fixture_reference(fixture_frames, name, clamp, 8.0, 0.05, 0), _fixture_reference(fixture_frames, name, clamp, 8.0, 0.05, LINEAR)
        assert not np.array_equal(a[1], b[1]) and rr.same_f32_or_nan(a[0], b[0]).all()          # the tone flags reach the RGBA8 plane alone
        assert not rr.same_f32_or_nan(a[0], _fixture_reference(fixture_frames, name, clamp, 1.0, 0.05, 0)[0]).all()
        assert not rr.same_f32_or_nan(a[0], _fixture_reference(fixture_frames, name, clamp, 8.0, 0.0, 0)[0]).all()
        assert not rr.same_f32_or_nan(a[0], _fixture_reference(fixture_frames, name, not clamp, 8.0, 0.05, 0)[0]).all()


# ---- 2. frame shapes ----

@pytest.mark.parametrize("shape", [(1, 1), (130, 1), (5, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_shapes(ctx, shape):
    w, h = shape
    arr, mats, tex = rq.field_world()
    prev_cam, cam = _look(w, h), second_cameras(w, h)["moved a little"]
    ctx.set_scene(hbm_worlds.scene_from_arrays(prev_cam, arr, mats, tex), hbm=True)
    p = _pt(w, h)
    prev_colour, prev_guides = _frame(ctx, prev_cam, p, 0)
    prev_colour = _with_lengths(prev_colour, 2)
    colour, guides = _frame(ctx, cam, p, 1)
    for clamp in (True, False):
        want = rr.reproject(colour, guides, prev_colour, prev_guides, prev_cam, cam, w, h, clamp=clamp)
        got = ctx.reproject(p, m.make_reproject_params(prev_cam, cam, max_history=8.0, clamp=clamp), colour, guides, prev_colour, prev_guides, rgba8=True)
        _same(got, want, f"{w} x {h}, clamp {clamp}")
    if h > 1:
        assert 0.0 < rr.history_fraction(want[0])


def test_a_band_of_rows_whose_projection_leaves_it_above_and_below(ctx):
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt(row_begin=7, row_end=29)
    full = _pt()
    ups = {"up": _look(W, H, EYE, (0, 1.5, 0)), "down": _look(W, H, EYE, (0, -0.5, 0))}       # the view tilts: the image moves by several rows
    prev_cam = _look(W, H)
    prev_colour, prev_guides = _frame(ctx, prev_cam, p, 0)
    assert prev_guides.shape == (22, W) and prev_colour.shape == (22, W, 4)
    prev_full = _frame(ctx, prev_cam, full, 0)
    for name, cam in ups.items():
        colour, guides = _frame(ctx, cam, p, 3)
        want = rr.reproject(colour, guides, prev_colour, prev_guides, prev_cam, cam, W, H, 7)
        got = ctx.reproject(p, m.make_reproject_params(prev_cam, cam, max_history=8.0), colour, guides, prev_colour, prev_guides, rgba8=True)
        _same(got, want, f"rows 7..29, tilted {name}")
        # the same rows of the whole frame find more history: there the taps above / below the band exist
        cf, gf = _frame(ctx, cam, full, 3)
        whole = rr.reproject(cf, gf, prev_full[0], prev_full[1], prev_cam, cam, W, H)[0][7:29]
        assert 0.0 < rr.history_fraction(want[0]) < rr.history_fraction(whole), name
    ctx.set_camera(prev_cam)


# ---- 3. the device form: a caller stream, 4-byte alignment, canaries; crafted frames ----

def _device_call(ctx, p, r, colour, guides, prev_colour, prev_guides, *, rgba8, stream=None, offset=4):
    """mirt_ctx_reproject_device with every plane `offset` bytes into an allocation of its own (4: 4-byte but not 16-byte aligned) and
    0x5A canaries around `out` and `out_rgba8` -> (out, rgba8 or None).  The inputs are read back and compared: the call writes none."""
    import torch
    n = guides.size
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        def up(a):
            t = torch.zeros(offset + a.nbytes + 16, dtype=torch.uint8, device="cuda:0")
            t[offset:offset + a.nbytes] = torch.from_numpy(_bytes(a).copy()).to("cuda:0")
            return t
        ins = [up(a) for a in (colour, guides, prev_colour, prev_guides)]
        d_out = torch.full((offset + 16 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_rgba = torch.full((offset + 4 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        st.synchronize()
        ctx.reproject_device(p, r, *(t.data_ptr() + offset for t in ins), d_out.data_ptr() + offset, n,
                             d_out_rgba8=d_rgba.data_ptr() + offset if rgba8 else None, stream=st.cuda_stream)
        st.synchronize()
        out, rgba = d_out.cpu().numpy(), d_rgba.cpu().numpy()
        back = [t.cpu().numpy() for t in ins]
    for a, b in zip((colour, guides, prev_colour, prev_guides), back):
        assert np.array_equal(b[offset:offset + a.nbytes], _bytes(a)) and not b[:offset].any() and not b[offset + a.nbytes:].any(), "an input was written"
    assert (out[:offset] == 0x5A).all() and (out[offset + 16 * n:] == 0x5A).all(), "bytes outside out were written"
    assert (rgba[:offset] == 0x5A).all() and (rgba[offset + 4 * n:] == 0x5A).all(), "bytes outside out_rgba8 were written"
    shape = guides.shape
    lin = out[offset:offset + 16 * n].copy().view(f32).reshape(shape + (4,))
    if not rgba8:
        assert (rgba == 0x5A).all(), "out_rgba8 was written though it was not passed"
        return lin, None
    return lin, rgba[offset:offset + 4 * n].copy().reshape(shape + (4,))


def test_the_device_form_on_a_caller_stream_at_4_byte_alignment(ctx, fixture_frames):
    import torch
    p, prev_colour, prev_guides, prev_cam, cur = fixture_frames
    colour, guides, cam = cur["moved a little"]
    stream = torch.cuda.Stream(device="cuda:0")
    for clamp in (True, False):
        want = _fixture_reference(fixture_frames, "moved a little", clamp, 8.0, 0.05, 0)
        r = m.make_reproject_params(prev_cam, cam, max_history=8.0, clamp=clamp)
        got = _device_call(ctx, p, r, colour, guides, prev_colour, prev_guides, rgba8=True, stream=stream)
        assert ctx.last_kernel() == f"reproject_kernel<{'true' if clamp else 'false'},true>"
        _same(got, want, f"device form, clamp {clamp}, with RGBA8")
        lin, none = _device_call(ctx, p, r, colour, guides, prev_colour, prev_guides, rgba8=False, stream=stream)
        assert none is None and ctx.last_kernel() == f"reproject_kernel<{'true' if clamp else 'false'},false>"
        assert rr.same_f32_or_nan(lin, want[0]).all()
    ctx.synchronize()


def _crafted(frames):
    """The fixture's real frames ("moved a little") with every branch of the rule written into them: NaN and infinite colours and
    guides, history lengths 0, 0.5, 1, 7 and NaN, MISS on either side, unequal ids."""
    _, prev_colour, prev_guides, prev_cam, cur = frames
    colour, guides, cam = cur["moved a little"]
    colour, guides, prev_colour, prev_guides = colour.copy(), guides.copy(), prev_colour.copy(), prev_guides.copy()
    rng = np.random.default_rng(23)
    prev_colour[..., 3] = rng.choice(np.array([0.0, 0.5, 1.0, 7.0, 7.0, 3.0, np.nan], f32), (H, W))
    guides["sphere"][3:6, 10:30] = MISS                               # a hit became a miss
    prev_guides["sphere"][20:24, 5:40] = MISS                         # ... and the other way round
    prev_guides["sphere"][30:33, :] += 1                              # unequal ids
    gt, pt = guides["t"], prev_guides["t"]
    gt[8, 8:14] = [np.nan, np.inf, -np.inf, -5.0, 0.0, 1e-30]
    pt[12, 8:14] = [np.nan, np.inf, -np.inf, -5.0, 0.0, 3e38]
    pt[25:28, 20:40] *= f32(1.04)                                     # inside a tolerance of 0.05, outside one of 0.02
    colour[10, 10:13, :3] = [[np.nan, np.inf, -np.inf], [3e38, -3e38, 0.0], [-0.0, 1e-40, 5.0]]
    colour[..., 3] = np.nan                                           # ignored
    prev_colour[15, 15:19, :3] = [[np.inf, np.nan, -np.inf], [3e38, 3e38, 3e38], [-1.0, -0.0, 1e-40], [np.nan, np.nan, np.nan]]
    prev_colour[15, 15:19, 3] = [7.0, np.inf, 3e38, 1.0]
    prev_colour[16, 15:19] = [np.inf, np.inf, np.inf, 0.5]            # infinite and too short: skipped, not weighted with 0
    return colour, guides, prev_colour, prev_guides, prev_cam, cam


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "no clamp"])
def test_crafted_frames(ctx, fixture_frames, clamp):
    colour, guides, prev_colour, prev_guides, prev_cam, cam = _crafted(fixture_frames)
    p = _pt()
    for mh, dt in ((8.0, 0.05), (1.0, 0.02), (2.0 ** 20, 0.0), (3.5, 10.0)):
        want = rr.reproject(colour, guides, prev_colour, prev_guides, prev_cam, cam, W, H, max_history=mh, depth_tolerance=dt, clamp=clamp)
        r = m.make_reproject_params(prev_cam, cam, max_history=mh, depth_tolerance=dt, clamp=clamp)
        _same(_device_call(ctx, p, r, colour, guides, prev_colour, prev_guides, rgba8=True), want, f"crafted, clamp {clamp}, max_history {mh}, depth_tolerance {dt}")
        _same(ctx.reproject(p, r, colour, guides, prev_colour, prev_guides, rgba8=True), want, f"crafted, host form, clamp {clamp}, max_history {mh}")
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and 0.2 < rr.history_fraction(want[0]) < 0.95
    # a scalar walk over a few rows that hold crafted records agrees with the planes (the whole small frame: tests/test_reproject_abi.py)
    rows = slice(14, 18)
    a = rr.reproject(colour[rows], guides[rows], prev_colour[rows], prev_guides[rows], prev_cam, cam, W, H, 14, clamp=clamp)
    b = rr.reproject_naive(colour[rows], guides[rows], prev_colour[rows], prev_guides[rows], prev_cam, cam, W, H, 14, clamp=clamp)
    assert rr.same_f32_or_nan(a[0], b[0]).all() and np.array_equal(a[1], b[1])


# ---- 4. the whole chain on one stream, on an HBM and on an LDS scene ----

@pytest.mark.parametrize("hbm", [True, False], ids=["HBM scene", "LDS scene"])
def test_the_chain_of_device_calls_on_one_stream(ctx, hbm):
    import torch
    ctx.set_scene(fr.fixture_scene(), hbm=hbm)
    n = W * H
    stream = torch.cuda.Stream(device="cuda:0")
    st = stream.cuda_stream
    cams = [_look(W, H), second_cameras()["moved a little"]]
    with torch.cuda.stream(stream):
        planes = {k: [torch.zeros(size * n, dtype=torch.uint8, device="cuda:0") for _ in range(2)] for k, size in (("guides", 32), ("history", 16))}
        colour = torch.zeros(16 * n, dtype=torch.uint8, device="cuda:0")
        img = torch.zeros(4 * n, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
    tone = _pt(spp=0)
    to_f32 = m.make_denoise_params("accum", levels=3, f32=True)
    host = []
    for k, cam in enumerate(cams):
        p = _pt(seed=40 + k)
        ctx.set_camera(cam)
        ctx.accum_reset(p)
        ctx.accum_frame_device(p, img.data_ptr(), st)
        ctx.render_features_device(p, planes["guides"][k].data_ptr(), 32 * n, stream=st, lds=not hbm)
        if k == 0:
            ctx.denoise_device(tone, to_f32, planes["guides"][0].data_ptr(), 32 * n, planes["history"][0].data_ptr(), 16 * n, st)
        else:
            ctx.denoise_device(tone, to_f32, planes["guides"][1].data_ptr(), 32 * n, colour.data_ptr(), 16 * n, st)
            ctx.reproject_device(tone, m.make_reproject_params(cams[0], cams[1], max_history=8.0), colour.data_ptr(), planes["guides"][1].data_ptr(),
                                 planes["history"][0].data_ptr(), planes["guides"][0].data_ptr(), planes["history"][1].data_ptr(), n,
                                 d_out_rgba8=img.data_ptr(), stream=st)
            assert ctx.last_kernel() == "reproject_kernel<true,true>"
        # (the host reads between the frames only to feed the reference: the chain of a frame has no host wait)
        stream.synchronize()
        sums, count = ctx.accum_read(p), ctx.accum_samples()
        guides = planes["guides"][k].cpu().numpy().view(FEATURE_DTYPE).reshape(H, W)
        assert np.array_equal(_bytes(guides), _bytes(ctx.render_features(p, lds=not hbm)))
        host.append((dr.denoise(sums, count, guides, 3, 1.0, 5)[0], guides))
    want = rr.reproject(host[1][0], host[1][1], host[0][0], host[0][1], cams[0], cams[1], W, H, max_history=8.0)
    got = (planes["history"][1].cpu().numpy().view(f32).reshape(H, W, 4), img.cpu().numpy().reshape(H, W, 4))
    _same(got, want, f"the chain, hbm {hbm}")
    assert rr.same_f32_or_nan(planes["history"][0].cpu().numpy().view(f32).reshape(H, W, 4), host[0][0]).all()
    assert 0.5 < rr.history_fraction(want[0]) < 1.0
    ctx.synchronize()
    ctx.set_camera(cams[0])


# ---- 5. what a call leaves alone; no scene at all ----

def test_a_call_changes_no_state(ctx, fixture_frames):
    p, prev_colour, prev_guides, prev_cam, cur = fixture_frames
    colour, guides, cam = cur["moved a little"]
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    q = _pt(seed=77)
    ctx.accum_reset(q)
    ctx.accum_frame(q)
    sums, n = ctx.accum_read(q), ctx.accum_samples()
    ctx.stats()                                                      # folds the launches so far: the next read counts from here
    stats = ctx.stats()
    assert stats["launches"] == 0
    r = m.make_reproject_params(prev_cam, cam, max_history=8.0)
    got = ctx.reproject(p, r, colour, guides, prev_colour, prev_guides, rgba8=True)
    assert ctx.last_kernel() == "reproject_kernel<true,true>"
    _same(got, _fixture_reference(fixture_frames, "moved a little", True, 8.0, 0.05, 0), "state")
    assert np.array_equal(ctx.accum_read(q), sums) and ctx.accum_samples() == n and ctx.stats() == stats
    ctx.accum_frame(q)                                               # the next frame continues the accumulation as if nothing had happened
    after = ctx.accum_read(q)
    ctx.accum_reset(q)
    ctx.accum_frame(q)
    ctx.accum_frame(q)
    assert np.array_equal(after, ctx.accum_read(q))


def test_a_context_without_a_scene_reprojects(fixture_frames):
    p, prev_colour, prev_guides, prev_cam, cur = fixture_frames
    colour, guides, cam = cur["moved a little"]
    with m.Context(0) as fresh:
        got = fresh.reproject(p, m.make_reproject_params(prev_cam, cam, max_history=8.0), colour, guides, prev_colour, prev_guides, rgba8=True)
        assert fresh.last_kernel() == "reproject_kernel<true,true>"
    _same(got, _fixture_reference(fixture_frames, "moved a little", True, 8.0, 0.05, 0), "no scene")


# ---- 6. every error code ----

def test_error_codes(ctx, fixture_frames):
    lib = m.lib()
    h = ctx._h
    p, prev_colour, prev_guides, prev_cam, cur = fixture_frames
    colour, guides, cam = cur["moved a little"]
    n = W * H
    planes = dict(colour=np.ascontiguousarray(colour), guides=np.ascontiguousarray(guides), prev_colour=np.ascontiguousarray(prev_colour),
                  prev_guides=np.ascontiguousarray(prev_guides), out=np.full((n + 1, 4), 7.0, f32), out_rgba8=np.full((n + 1, 4), 0xA5, np.uint8))
    good = m.make_reproject_params(prev_cam, cam)

    def call(params=p, r=good, pixels=n, **ptr):
        f = _abi.MirtReprojectFrames()
        for k, a in planes.items():
            setattr(f, k, ptr.get(k, a.ctypes.data))
        f.pixels = pixels
        pp = C.byref(params) if params is not None else None
        rp = C.byref(r) if r is not None else None
        host = lib.mirt_ctx_reproject(h, pp, rp, C.byref(f))
        dev = lib.mirt_ctx_reproject_device(h, pp, rp, C.byref(f), None)      # (refused before any pointer is used: host memory does no harm)
        assert host == dev, (host, dev)
        return host

    def with_(**kw):
        r = m.make_reproject_params(prev_cam, cam)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    E = _abi
    assert call(params=None) == call(r=None) == E.MIRT_ERR_NULL_POINTER
    assert lib.mirt_ctx_reproject(h, C.byref(p), C.byref(good), None) == lib.mirt_ctx_reproject_device(h, C.byref(p), C.byref(good), None, None) == E.MIRT_ERR_NULL_POINTER
    for k in ("colour", "guides", "prev_colour", "prev_guides", "out"):
        assert call(**{k: None}) == E.MIRT_ERR_NULL_POINTER, k
    assert call(r=with_(flags=2), colour=None) == E.MIRT_ERR_NULL_POINTER                        # the order of the checks
    for kw in (dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(max_history=0.5), dict(max_history=0.0), dict(max_history=-8.0),
               dict(max_history=float("nan")), dict(max_history=float("inf")), dict(depth_tolerance=-0.01), dict(depth_tolerance=float("nan")),
               dict(depth_tolerance=float("inf"))):
        assert call(r=with_(**kw)) == E.MIRT_ERR_BAD_MODE, kw
    assert call(params=_pt(0, H), r=with_(flags=2)) == E.MIRT_ERR_BAD_MODE
    assert call(params=_pt(0, H)) == call(params=_pt(W, 0)) == E.MIRT_ERR_VIEWPORT_SIZE
    assert call(params=_pt(row_begin=30, row_end=20)) == call(params=_pt(row_begin=0, row_end=H + 1)) == E.MIRT_ERR_BAD_ROWS
    assert call(params=_pt(tile_rows=4, n_parts=3, part=1)) == E.MIRT_ERR_BAD_ROWS             # a tile partition
    assert call(params=_pt(tile_rows=4, n_parts=3, part=1), pixels=0) == E.MIRT_ERR_BAD_ROWS   # ... before the buffers
    assert call(pixels=n - 1) == call(pixels=0) == call(params=_pt(W + 1, H)) == E.MIRT_ERR_OUT_BUFFER
    out, rgba = planes["out"], planes["out_rgba8"]
    for k, size in (("colour", 16), ("guides", 32), ("prev_colour", 16), ("prev_guides", 32)):
        a = planes[k]
        assert call(out=a.ctypes.data) == call(out_rgba8=a.ctypes.data) == E.MIRT_ERR_OUT_BUFFER, k
        assert call(out=a.ctypes.data + size * n - 4) == call(out_rgba8=a.ctypes.data + size * n - 4) == E.MIRT_ERR_OUT_BUFFER, k      # the last word
        assert call(**{k: out.ctypes.data + 16 * n - 4}) == call(**{k: rgba.ctypes.data + 4 * n - 4}) == E.MIRT_ERR_OUT_BUFFER, k
    assert call(out_rgba8=out.ctypes.data + 16) == call(out=rgba.ctypes.data) == E.MIRT_ERR_OUT_BUFFER
    assert (out == 7.0).all() and (rgba == 0xA5).all(), "a refused call wrote to an output"
    assert b"overlap" in lib.mirt_last_error()
    assert call(params=_pt(row_begin=9, row_end=9), pixels=0) == E.MIRT_ERR_BAD_ROWS            # an empty band is no band (as for a render)
    # the largest and the smallest parameters the rule accepts run
    for mh, dt in ((1.0, 0.0), (3.0e38, 3.0e38)):
        want = rr.reproject(colour, guides, prev_colour, prev_guides, prev_cam, cam, W, H, max_history=mh, depth_tolerance=dt)
        _same(ctx.reproject(p, m.make_reproject_params(prev_cam, cam, max_history=mh, depth_tolerance=dt), colour, guides, prev_colour, prev_guides, rgba8=True), want,
              f"max_history {mh}, depth_tolerance {dt}")


# ---- 7. Raytracer.temporal_frame ----

TW, TH = 96, 64


def _pose(k):
    fly = m.FlyCameraController.default()
    fly.position = np.array([-10.0, 2.0 + 0.03 * k, -4.0 + 0.1 * k], f32)
    fly.yaw = m.Angle.degrees(25.0 + 0.4 * k)
    fly.aperture = 0.0
    return fly.renderer_camera()


def _render_params(k):
    return m.RenderParams(camera=_pose(k), viewport_size=(TW, TH), sampling=m.SamplingParams(max_samples_per_pixel=8, num_samples_per_pixel=2, num_bounces=8))


def _by_hand(rt, seed, flags=0):
    """One frame of `rt` through the blocking calls: (denoised float32, denoised RGBA8, guides, the camera)."""
    ctx = rt._ctx
    p = rt._params(2, seed, flags)
    ctx.set_camera(rt.camera.c)
    ctx.accum_reset(p)
    ctx.accum_frame(p)
    g = rt.features(seed=seed, lds=True)
    guides = np.zeros((TH, TW), FEATURE_DTYPE)
    for k in g:
        guides[k] = g[k]
    tone = _pt(TW, TH, 0, flags=flags)
    return (ctx.denoise(tone, m.make_denoise_params("accum", f32=True), guides), ctx.denoise(tone, m.make_denoise_params("accum"), guides), guides,
            _abi.MirtGpuCamera.from_buffer_copy(rt.camera.c))


def test_temporal_frame_over_a_pan_is_the_steps_done_by_hand():
    scene, _ = m.scenes.three_spheres()
    rt, hand = (m.Raytracer(scene, _render_params(0), device=0) for _ in range(2))
    try:
        assert not rt._hbm and rt.temporal_history() is None
        history = prev = None
        for k in range(4):
            if k:
                rt.set_render_params(_render_params(k))              # a new camera keeps the history
                hand.set_render_params(_render_params(k))
            got = rt.temporal_frame(seed=5)
            colour, rgba, guides, cam = _by_hand(hand, 5 + k)
            if k == 0:
                history, want = colour, rgba
            else:
                r = m.make_reproject_params(prev[1], cam)
                history, want = hand._ctx.reproject(_pt(TW, TH, 0), r, colour, guides, history, prev[0], rgba8=True)
            assert got.shape == (TH, TW, 4) and got.dtype == np.uint8 and np.array_equal(got, want), k
            assert rr.same_f32_or_nan(rt.temporal_history(), history).all(), k
            if k:                                                    # ... and the reference's, with the wrappers' defaults
                ref = rr.reproject(colour, guides, before, prev[0], prev[1], cam, TW, TH, max_history=4.0, depth_tolerance=0.05, clamp=True)
                _same((history, want), ref, f"temporal frame {k}")
            before, prev = history, (guides, cam)
            assert rt._accumulated is None and not rt._hbm
        lengths = rt.temporal_history()[..., 3]
        assert lengths.max() == 4.0 and (lengths > 1).mean() > 0.8           # four frames: the cap of max_history = 4 is reached
        # a progressive loop restarts behind it
        first = rt.render_frame(seed=1)
        assert rt._ctx.accum_samples() == 2 and first.shape == (TH, TW, 4)
        # the parameters reach the calls
        rt.temporal_frame(seed=5, max_history=2.0, clamp=False, flags=LINEAR)
        assert rt.temporal_history()[..., 3].max() == 2.0 and rt._ctx.last_kernel() == "reproject_kernel<false,true>"
        # set_world drops the history: the next frame is the denoised frame alone
        rt.set_world(scene.spheres)
        hand.set_world(scene.spheres)
        got = rt.temporal_frame(seed=5)
        colour, rgba, guides, cam = _by_hand(hand, 5 + 5)
        assert np.array_equal(got, rgba) and (rt.temporal_history()[..., 3] == 1).all() and rr.same_f32_or_nan(rt.temporal_history(), colour).all()
        rt.temporal_frame(seed=5)
        assert (rt.temporal_history()[..., 3] > 1).mean() > 0.8
        rt.move_spheres(1, [scene.spheres[1]])                       # ... and so does move_spheres
        rt.temporal_frame(seed=5)
        assert (rt.temporal_history()[..., 3] == 1).all()
        # ... and a changed viewport size
        rt.set_render_params(m.RenderParams(camera=_pose(3), viewport_size=(80, 48), sampling=_render_params(3).sampling))
        assert rt.temporal_frame(seed=5).shape == (48, 80, 4) and (rt.temporal_history()[..., 3] == 1).all()
        with pytest.raises(ValueError):
            rt.temporal_frame(flags=m.MIRT_FLAG_COUNT_WORK)
        with pytest.raises(ValueError):
            rt.temporal_frame(max_history="4")
    finally:
        rt.close()
        hand.close()


def test_temporal_frame_refuses_a_node():
    scene, _ = m.scenes.three_spheres()
    rt = m.Raytracer(scene, _render_params(0), devices=[0, 0])
    try:
        with pytest.raises(ValueError):
            rt.temporal_frame()
    finally:
        rt.close()
