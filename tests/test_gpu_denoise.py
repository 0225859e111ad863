"""mirt_ctx_denoise* on the device against tests/denoise_ref.py: every comparison is the float32 output bit for bit AND the RGBA8
bytes.  The sums come from real progressive frames (read back with mirt_ctx_accum_read) or from records written with
mirt_ctx_adapt_write, the guides from mirt_ctx_render_features or crafted by hand, so the filter is the only thing under test.  One
context for the module; a reference is computed once per (frame, parameters)."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import ADAPT_PIXEL_DTYPE, FEATURE_DTYPE
import adaptive_ref as ar
import denoise_ref as dr
import feature_ref as fr
import hbm_worlds
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = dr.MISS
LINEAR = m.MIRT_FLAG_NO_TONEMAP | m.MIRT_FLAG_NO_SRGB
W, H = fr.W, fr.H


def _name(levels, out):
    """The kernel of the LAST level: levels 0 .. 3 (steps 1 .. 8) run the staged shape, levels 4 .. 7 the direct one."""
    return f"denoise_atrous_{'staged_' if levels <= 4 else ''}kernel<{out}>"


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _pt(w=W, h=H, spp=2, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, **kw)


def _same(got_f32, got_rgba, want, what):
    wf, wr = want
    assert got_f32.shape == wf.shape and got_f32.dtype == f32 and got_rgba.shape == wr.shape and got_rgba.dtype == np.uint8, what
    bad = np.argwhere((got_f32.view(np.uint32) != wf.view(np.uint32)).any(-1))
    bad8 = np.argwhere((got_rgba != wr).any(-1))
    print(f"{what}: {wf.shape[0] * wf.shape[1]} pixels, {len(bad)} float32 records and {len(bad8)} RGBA8 pixels differ")
    assert len(bad) == 0, f"{what}: float32 differs at {bad[0]}: got {got_f32[tuple(bad[0])]}, want {wf[tuple(bad[0])]}"
    assert len(bad8) == 0, f"{what}: RGBA8 differs at {bad8[0]}: got {got_rgba[tuple(bad8[0])]}, want {wr[tuple(bad8[0])]}"


def _both(ctx, p, source, guides, levels, sigma, nl):
    """The two output forms of one host call each."""
    got = ctx.denoise(p, m.make_denoise_params(source, levels=levels, sigma_colour=sigma, normal_log2=nl, f32=True), guides)
    assert ctx.last_kernel() == _name(levels, "f32")
    rgba = ctx.denoise(p, m.make_denoise_params(source, levels=levels, sigma_colour=sigma, normal_log2=nl), guides)
    assert ctx.last_kernel() == _name(levels, "rgba8")
    return got, rgba


def _accumulate(ctx, p, frames=2):
    """`frames` progressive frames of p.spp samples -> (sums uint64 [rows, w, 3], the count)."""
    ctx.accum_reset(p)
    for _ in range(frames):
        ctx.accum_frame(p)
    return ctx.accum_read(p), ctx.accum_samples()


# ---- 1. the fixture frame: 67 x 45, neither a multiple of a tile nor of a wave ----

@pytest.fixture(scope="module")
def fixture_frame(ctx):
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt()
    sums, n = _accumulate(ctx, p)
    guides = ctx.render_features(p)
    assert n == 4 and sums.any() and (guides["sphere"] == MISS).sum() > 500 and (guides["sphere"] != MISS).sum() > 1000
    for a in (sums, guides):
        a.setflags(write=False)
    return p, sums, n, guides


_references = {}


def _fixture_reference(frame, levels, sigma, nl, flags):
    key = (levels, sigma, nl, flags)
    if key not in _references:
        _, sums, n, guides = frame
        _references[key] = dr.denoise(sums, n, guides, levels, sigma, nl, flags)
    return _references[key]


@pytest.mark.parametrize("nl", [0, 5])
@pytest.mark.parametrize("sigma", [0.0, 1.0])
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_the_fixture_frame_matches_the_reference(ctx, fixture_frame, levels, sigma, nl):
    p, sums, n, guides = fixture_frame
    assert ctx.accum_samples() == n
    got = _both(ctx, p, "accum", guides, levels, sigma, nl)
    _same(*got, _fixture_reference(fixture_frame, levels, sigma, nl, 0), f"levels {levels}, sigma {sigma}, normal_log2 {nl}")
    st = ctx.trace_stats()
    assert st["kernel_ms"] > 0.0
    if levels == 3:                                                  # the tone flags reach the epilogue
        for flags in (m.MIRT_FLAG_NO_TONEMAP, m.MIRT_FLAG_NO_SRGB, LINEAR):
            q = _pt(flags=flags)
            want = _fixture_reference(fixture_frame, levels, sigma, nl, flags)
            _same(*_both(ctx, q, "accum", guides, levels, sigma, nl), want, f"levels 3, sigma {sigma}, normal_log2 {nl}, flags {flags}")
            assert not np.array_equal(want[1], got[1])


@pytest.mark.parametrize("mask", [0, 255], ids=["every level direct", "every level staged"])
def test_either_shape_gives_the_same_bytes_at_every_level(fixture_frame, monkeypatch, mask):
    """MIRT_DENOISE_STAGED (read when a context is created) forces a shape: steps 16 .. 128 staged and steps 1 .. 8 direct are not what a
    default call runs, and their bytes are the reference's too."""
    p, sums, n, guides = fixture_frame
    monkeypatch.setenv("MIRT_DENOISE_STAGED", str(mask))
    with m.Context(0) as c2:
        c2.set_scene(fr.fixture_scene(), hbm=True)
        assert np.array_equal(_accumulate(c2, p)[0], sums)
        for levels in (3, 8):
            d = dict(levels=levels, sigma_colour=1.0, normal_log2=5)
            got = c2.denoise(p, m.make_denoise_params("accum", f32=True, **d), guides)
            assert c2.last_kernel() == f"denoise_atrous_{'staged_' if mask else ''}kernel<f32>"
            rgba = c2.denoise(p, m.make_denoise_params("accum", **d), guides)
            want = _fixture_reference(fixture_frame, levels, 1.0, 5, 0)
            _same(got, rgba, want, f"mask {mask}, levels {levels}")


def test_the_filter_changes_the_frame_and_keeps_it_finite(ctx, fixture_frame):
    p, sums, n, guides = fixture_frame
    got, _ = _both(ctx, p, "accum", guides, 3, 1.0, 5)
    raw = dr.means(sums, n)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all() and not np.array_equal(got[..., :3], raw)


# ---- 2. frame shapes ----

@pytest.mark.parametrize("shape", [(1, 1), (130, 1), (5, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_shapes(ctx, shape):
    w, h = shape
    arr, mats, tex = rq.field_world()
    ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25), arr, mats, tex), hbm=True)
    p = _pt(w, h)
    sums, n = _accumulate(ctx, p, 1)
    guides = ctx.render_features(p)
    for levels in (1, 5):
        _same(*_both(ctx, p, "accum", guides, levels, 1.0, 5), dr.denoise(sums, n, guides, levels, 1.0, 5), f"{w} x {h}, levels {levels}")


def test_a_band_of_rows(ctx):
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt(row_begin=7, row_end=29)
    sums, n = _accumulate(ctx, p, 1)
    guides = ctx.render_features(p)
    assert guides.shape == (22, W) and sums.shape == (22, W, 3)
    _same(*_both(ctx, p, "accum", guides, 5, 1.0, 5), dr.denoise(sums, n, guides, 5, 1.0, 5), "rows 7..29")


# ---- 3. crafted records and crafted guides ----

CW, CH = 37, 11


def _crafted():
    """Records and guide sets at the corners of the rule."""
    rng = np.random.default_rng(17)
    n = CW * CH
    rec = np.zeros(n, ADAPT_PIXEL_DTYPE)
    rec["sum"] = rng.integers(0, 3 << 20, (n, 3)).astype(np.uint64) * rng.integers(1, 9, (n, 1)).astype(np.uint64)
    rec["samples"] = rng.integers(1, 9, n)
    rec["even"] = rec["sum"] // 2
    rec["samples"][::7] = 0                                          # n == 0 pixels: mean 0, whatever the sums say
    rec["sum"][5] = 2 ** 64 - 1                                      # the largest record mirt_ctx_adapt_write can install
    rec["samples"][5] = 1
    rec["sum"][40:44] = 2 ** 64 - 1
    rec["samples"][40:44] = 1
    base = np.zeros((CH, CW), FEATURE_DTYPE)
    base["albedo"] = rng.uniform(0.05, 1.0, (CH, CW, 3)).astype(f32)
    nrm = rng.normal(size=(CH, CW, 3))
    base["normal"] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(f32)
    base["t"] = 1.0
    sets = {}
    g = base.copy(); g["sphere"] = np.arange(n).reshape(CH, CW); sets["all ids distinct"] = g
    g = base.copy(); g["sphere"] = MISS; sets["all MISS"] = g
    ys, xs = np.divmod(np.arange(n), CW)
    g = base.copy(); g["sphere"] = (((xs // 3) + (ys // 2)) & 1).reshape(CH, CW) + 7; sets["a checker of two ids"] = g
    g = base.copy(); g["sphere"] = 3
    flat = g.reshape(-1)
    flat["albedo"][0::11] = [np.nan, np.inf, -np.inf]
    flat["albedo"][1::11] = [-1.0, 0.0, -0.0]
    flat["albedo"][2::11] = [1e30, 3.0e38, 64.0]
    flat["albedo"][3::11] = [0.015625, np.nextafter(f32(0.015625), f32(0)), np.nextafter(f32(64.0), f32(100))]
    flat["albedo"][4::11] = [1e-40, 1e-9, 65.0]
    flat["normal"][5::11] = [np.nan, 0.0, 1.0]
    flat["normal"][6::11] = [np.inf, -np.inf, 0.0]
    flat["normal"][7::11] = [1e30, 1e30, 1e30]
    flat["normal"][8::11] = [-1.0, 0.0, 0.0]
    flat["normal"][9::11] = [0.0, 0.0, 0.0]
    flat["sphere"][10::22] = MISS                                    # a miss keeps its albedo out of the divisor
    sets["NaN, infinite, negative and huge albedos and normals"] = g
    return rec, sets


@pytest.fixture(scope="module")
def crafted(ctx):
    """A context whose adaptive buffer has seen one step (the resolves' condition) and then holds the crafted records."""
    ctx.set_scene(ar.scene(w=CW, h=CH), hbm=True)
    p = ar.params(spp=2, w=CW, h=CH)
    ctx.adapt_reset(p)
    ctx.adapt_step(p, m.make_adapt_params(2, 2, 0))
    rec, sets = _crafted()
    ctx.adapt_write(rec)
    return p, rec, sets


@pytest.mark.parametrize("name", ["all ids distinct", "all MISS", "a checker of two ids", "NaN, infinite, negative and huge albedos and normals"])
def test_crafted_records_and_guides(ctx, crafted, name):
    p, rec, sets = crafted
    guides = sets[name]
    sums, n = rec["sum"].reshape(CH, CW, 3), rec["samples"].reshape(CH, CW)
    for levels, sigma, nl in ((3, 1.0, 5), (5, 0.0, 8), (2, 1e-3, 0), (8, 1e3, 1)):
        want = dr.denoise(sums, n, guides, levels, sigma, nl)
        assert np.isfinite(want[0]).all()
        _same(*_both(ctx, p, "adapt", guides, levels, sigma, nl), want, f"{name}: levels {levels}, sigma {sigma}, normal_log2 {nl}")
    if name == "all ids distinct":                                   # no neighbour has any weight: the frame is the mean itself
        got, _ = _both(ctx, p, "adapt", guides, 3, 1.0, 5)
        den = dr.divisors(guides)
        c = (dr.means(sums, n) / den).astype(f32)
        for _ in range(3):
            c = ((f32(36.0) * c).astype(f32) / f32(36.0)).astype(f32)
        assert dr.same_f32(got[..., :3], (c * den).astype(f32))
    assert np.array_equal(_bytes(ctx.adapt_read()), _bytes(rec))      # the records are read, never written


# ---- 4. the accumulation of a scene that lives in LDS, guides from MIRT_QUERY_LDS ----

def test_the_accumulation_of_a_scene_in_lds(ctx, fixture_frame):
    ctx.set_scene(fr.fixture_scene())                                # 3000 spheres: the LDS grid
    p = _pt()
    sums, n = _accumulate(ctx, p)
    assert "hbm" not in ctx.last_kernel()
    guides = ctx.render_features(p, lds=True)
    assert ctx.last_kernel().startswith("feature_frame_lds_kernel")
    assert np.array_equal(_bytes(guides), _bytes(fixture_frame[3]))  # the HBM twin's guides, and its sums
    assert np.array_equal(sums, fixture_frame[1])
    _same(*_both(ctx, p, "accum", guides, 3, 1.0, 5), dr.denoise(sums, n, guides, 3, 1.0, 5), "LDS scene")


# ---- 5. the device form: a caller stream, 4-byte alignment, canaries ----

def test_the_device_form_on_a_caller_stream(ctx, fixture_frame):
    import torch
    p, sums, n, guides = fixture_frame
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    assert _accumulate(ctx, p)[1] == n
    npix = W * H
    stream = torch.cuda.Stream(device="cuda:0")
    want = dr.denoise(sums, n, guides, 3, 1.0, 5)
    for f32_out, px in ((True, 16), (False, 4)):
        with torch.cuda.stream(stream):
            d_g = torch.zeros(4 + 32 * npix, dtype=torch.uint8, device="cuda:0")
            d_g[4:] = torch.from_numpy(_bytes(guides).copy()).to("cuda:0")
            d_out = torch.full((4 + px * npix + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
            ctx.denoise_device(p, m.make_denoise_params("accum", levels=3, f32=f32_out), d_g.data_ptr() + 4, 32 * npix, d_out.data_ptr() + 4, px * npix,
                               stream=stream.cuda_stream)
            stream.synchronize()
            host = d_out.cpu().numpy()
            back = d_g.cpu().numpy()
        assert (host[:4] == 0x5A).all() and (host[4 + px * npix:] == 0x5A).all(), "bytes outside the output were written"
        assert np.array_equal(back[4:], _bytes(guides)) and not back[:4].any(), "the guides were written"
        got = host[4:4 + px * npix].copy()
        if f32_out:
            assert dr.same_f32(got.view(f32).reshape(H, W, 4), want[0])
        else:
            assert np.array_equal(got.reshape(H, W, 4), want[1])
    ctx.synchronize()


# ---- 6. the scratch: reuse and growth ----

def test_scratch_reuse_and_growth(ctx):
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    frames = {}
    for w, h in ((16, 9), (200, 120)):
        cam = hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25)
        ctx.set_camera(cam)
        p = _pt(w, h)
        sums, n = _accumulate(ctx, p, 1)
        frames[(w, h)] = (p, sums, n, ctx.render_features(p))
    seen = {}
    with m.Context(0) as c2:                                         # a context whose scratch starts empty
        c2.set_scene(fr.fixture_scene(), hbm=True)
        for w, h in ((16, 9), (200, 120), (16, 9), (200, 120), (16, 9)):
            p, sums, n, guides = frames[(w, h)]
            c2.set_camera(hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25))
            assert np.array_equal(_accumulate(c2, p, 1)[0], sums)
            got = _both(c2, p, "accum", guides, 4, 1.0, 5)
            if (w, h) not in seen:
                seen[(w, h)] = got
                _same(*got, dr.denoise(sums, n, guides, 4, 1.0, 5), f"{w} x {h}")
            assert dr.same_f32(got[0], seen[(w, h)][0]) and np.array_equal(got[1], seen[(w, h)][1]), (w, h)
    ctx.set_camera(fr.fixture_camera())


# ---- 7. what a call leaves alone ----

def test_a_call_changes_no_state(ctx, crafted):
    import torch
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt()
    sums, n = _accumulate(ctx, p)
    ctx.stats()                                                      # folds the launches so far: the next read counts from here
    stats, records = ctx.stats(), ctx.adapt_read()
    assert stats["launches"] == 0
    guides = ctx.render_features(p)
    d_g = torch.from_numpy(_bytes(guides).copy()).to("cuda:0")
    d_out = torch.zeros(16 * W * H, dtype=torch.uint8, device="cuda:0")
    ctx.denoise_device(p, m.make_denoise_params("accum", levels=5, f32=True), d_g.data_ptr(), d_g.numel(), d_out.data_ptr(), d_out.numel())
    assert ctx.last_kernel() == _name(5, "f32")
    ctx.synchronize()                                                # the context's own stream: synchronize waits for the filter
    assert dr.same_f32(d_out.cpu().numpy().view(f32).reshape(H, W, 4), dr.denoise(sums, n, guides, 5, 1.0, 5)[0])
    assert np.array_equal(d_g.cpu().numpy(), _bytes(guides))
    assert np.array_equal(ctx.accum_read(p), sums) and ctx.accum_samples() == n
    assert ctx.stats() == stats
    assert np.array_equal(_bytes(ctx.adapt_read()), _bytes(records))
    # ... and the next frame continues the accumulation as if nothing had happened
    ctx.accum_frame(p)
    after = ctx.accum_read(p)
    assert np.array_equal(after, _accumulate(ctx, p, 3)[0])


# ---- 8. an ACCUM denoise is a link of the frame chain ----

def test_a_frame_on_the_other_stream_waits_for_the_filter(ctx):
    import torch
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    w, h = 320, 200                                                  # large enough for the filter to be running when the frame is queued
    cam = hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25)
    ctx.set_camera(cam)
    p = _pt(w, h)
    guides = ctx.render_features(p)
    want_sums = _accumulate(ctx, p, 3)[0]                            # the unfiltered loop: three frames
    sums2, n2 = _accumulate(ctx, p, 2)
    s0, s1 = ctx.frame_stream(0), ctx.frame_stream(1)
    d_g = torch.from_numpy(_bytes(guides).copy()).to("cuda:0")
    d_f = torch.zeros(16 * w * h, dtype=torch.uint8, device="cuda:0")
    d_img = torch.zeros(4 * w * h, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.denoise_device(p, m.make_denoise_params("accum", levels=8, f32=True), d_g.data_ptr(), d_g.numel(), d_f.data_ptr(), d_f.numel(), stream=s0)
    ctx.accum_frame_device(p, d_img.data_ptr(), stream=s1)           # rewrites the sums the filter reads: ordered behind it on the device
    ctx.synchronize()
    torch.cuda.synchronize()
    assert dr.same_f32(d_f.cpu().numpy().view(f32).reshape(h, w, 4), dr.denoise(sums2, n2, guides, 8, 1.0, 5)[0]), "the filter saw sums of the next frame"
    assert np.array_equal(ctx.accum_read(p), want_sums) and ctx.accum_samples() == 6
    ctx.accum_reset(p)                                               # a reset waits for a filter on a caller stream too
    ctx.set_camera(fr.fixture_camera())


# ---- 9. every error code ----

def test_error_codes(ctx, crafted):
    lib = m.lib()
    h = ctx._h
    ctx.set_scene(fr.fixture_scene(), hbm=True)
    p = _pt()
    sums, n = _accumulate(ctx, p)
    guides = np.ascontiguousarray(ctx.render_features(p))
    out = np.full(16 * W * H + 16, 0xA5, np.uint8)
    pg, po = C.c_void_p(guides.ctypes.data), C.c_void_p(out.ctypes.data)

    def call(params=p, d=None, g=pg, gl=guides.nbytes, o=po, ol=16 * W * H, **kw):
        d = d if d is not None else m.make_denoise_params(kw.pop("source", "accum"), f32=True, **kw)
        host = lib.mirt_ctx_denoise(h, C.byref(params) if params is not None else None, C.byref(d) if d is not False else None, g, gl, o, ol)
        dev = lib.mirt_ctx_denoise_device(h, C.byref(params) if params is not None else None, C.byref(d) if d is not False else None, g, gl, o, ol, None)
        assert host == dev, (host, dev)
        return host

    E = _abi
    assert call(params=None) == call(d=False) == call(g=None) == call(o=None) == E.MIRT_ERR_NULL_POINTER
    bad = m.make_denoise_params("accum"); bad.source = 2
    assert call(d=bad) == E.MIRT_ERR_BAD_MODE
    bad = m.make_denoise_params("accum"); bad.flags = 2
    assert call(d=bad) == E.MIRT_ERR_BAD_MODE
    for kw in (dict(levels=0), dict(levels=9), dict(normal_log2=9), dict(sigma_colour=-1.0), dict(sigma_colour=float("nan")), dict(sigma_colour=-0.5),
               dict(sigma_colour=1e-30), dict(sigma_colour=1e30), dict(sigma_colour=float("inf")), dict(sigma_colour=5e-18, levels=8)):
        assert "sigma_colour" not in kw or not dr.scales_valid(kw["sigma_colour"], kw.get("levels", 3)), kw
        assert call(**kw) == E.MIRT_ERR_BAD_MODE, kw
    assert call(params=_pt(tile_rows=4, n_parts=3, part=1)) == E.MIRT_ERR_BAD_ROWS
    assert call(params=_pt(tile_rows=4, n_parts=3, part=1), levels=0) == E.MIRT_ERR_BAD_MODE      # the order of the checks
    assert call(params=_pt(W + 1, H)) == call(params=_pt(row_begin=1)) == call(params=_pt(W, H + 1)) == E.MIRT_ERR_OUT_BUFFER
    assert call(gl=guides.nbytes - 1) == call(ol=16 * W * H - 1) == E.MIRT_ERR_OUT_BUFFER
    assert call(source="adapt") == E.MIRT_ERR_OUT_BUFFER             # the adaptive buffer is the crafted one: 37 x 11
    ctx.accum_reset(p)
    assert call() == E.MIRT_ERR_NO_SCENE                             # nothing accumulated
    assert (out == 0xA5).all(), "a refused call wrote to the output"
    with m.Context(0) as fresh:                                      # no buffer of either source
        for source in ("accum", "adapt"):
            with pytest.raises(m.MirtError) as e:
                fresh.denoise(p, m.make_denoise_params(source), guides)
            assert e.value.status == E.MIRT_ERR_OUT_BUFFER
        fresh.set_scene(fr.fixture_scene(), hbm=True)
        fresh.adapt_reset(p)
        with pytest.raises(m.MirtError) as e:                        # no step since the reset
            fresh.denoise(p, m.make_denoise_params("adapt"), guides)
        assert e.value.status == E.MIRT_ERR_NO_SCENE
    # the smallest and the largest sigma_colour the rule accepts at these levels run
    sums, n = _accumulate(ctx, p, 1)
    for sigma, levels in ((1e-18, 3), (1e18, 3), (2e-17, 8), (5e-18, 3)):
        assert dr.scales_valid(sigma, levels)
        _same(*_both(ctx, p, "accum", guides, levels, sigma, 5), dr.denoise(sums, n, guides, levels, sigma, 5), f"sigma {sigma}, levels {levels}")


# ---- 10. Raytracer.denoised ----

def test_raytracer_denoised_on_both_sources():
    scene, cam = m.scenes.three_spheres()
    rp = m.RenderParams(camera=cam, viewport_size=(96, 64), sampling=m.SamplingParams(max_samples_per_pixel=8, num_samples_per_pixel=2, num_bounces=8))
    rt = m.Raytracer(scene, rp, device=0)
    try:
        assert not rt._hbm                                           # three spheres live in LDS, and stay there
        for _ in range(2):
            rt.render_frame(seed=5)
        p = rt._params(0, 5, 0)
        sums, n = rt._ctx.accum_read(p), rt._ctx.accum_samples()
        g = rt.features(seed=5, lds=True)
        guides = np.zeros((64, 96), FEATURE_DTYPE)
        for k in g:
            guides[k] = g[k]
        want = dr.denoise(sums, n, guides, 3, 1.0, 5)
        assert dr.same_f32(rt.denoised(f32=True), want[0]) and np.array_equal(rt.denoised(), want[1])
        assert not rt._hbm and rt._ctx.accum_samples() == n == 4
        want4 = dr.denoise(sums, n, guides, 4, 0.5, 3, LINEAR)
        assert np.array_equal(rt.denoised(levels=4, sigma_colour=0.5, normal_log2=3, flags=LINEAR), want4[1])
        img, counts = rt.render_adaptive(64, 8, step=2, min_spp=2, seed=5, lds=True)
        rec = rt._ctx.adapt_read()
        want = dr.denoise(rec["sum"].reshape(64, 96, 3), rec["samples"].reshape(64, 96), guides, 3, 1.0, 5)
        assert dr.same_f32(rt.denoised("adapt", f32=True), want[0]) and np.array_equal(rt.denoised("adapt"), want[1])
        assert np.array_equal(rt._ctx.adapt_read()["samples"].reshape(64, 96), counts) and not rt._hbm
    finally:
        rt.close()
