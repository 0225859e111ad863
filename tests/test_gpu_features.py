"""mirt_ctx_render_features* on the device: feature_frame_kernel<true> (the BVH walk) and <false> (the flat scan) against the CPU
restatement in tests/feature_ref.py, pixel by pixel and bit by bit, for a host-built and a device-built tree.  One context for the
module; the reference computes a layer (one ray per pixel of a viewport) once and shares it among the frames that need it."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import FEATURE_DTYPE
import feature_ref as fr
import hbm_worlds
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

f32 = np.float32
MISS = fr.MISS
SEED = 0x1234_5678_9ABC                    # both halves of the 64-bit seed are mixed in
BVH = pytest.mark.parametrize("bvh", ["host", "device"])


@pytest.fixture(scope="module")
def ctx():
    c = m.Context(0)
    yield c
    c.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _set(ctx, scene, bvh="host"):
    ctx.set_scene(scene, hbm=True, bvh=bvh)
    assert ctx.bvh_info()["built_on_device"] == (bvh == "device")


def _tree_and_flat(ctx, params, what):
    """The tree's records [rows, width], after checking that the flat scan on the device returns the same bytes."""
    tree = ctx.render_features(params)
    assert ctx.last_kernel() == "feature_frame_kernel<true>"
    flat = ctx.render_features(params, flat=True)
    assert ctx.last_kernel() == "feature_frame_kernel<false>"
    assert tree.dtype == FEATURE_DTYPE and tree.shape == flat.shape == (m.params_out_rows(params), params.width)
    differ = np.argwhere((_bytes(tree).reshape(tree.shape + (32,)) != _bytes(flat).reshape(tree.shape + (32,))).any(-1))
    print(f"{what}: tree and flat differ in {len(differ)} of {tree.size} records")
    assert len(differ) == 0, f"{what}: tree != flat at compact pixel {differ[0]}: tree {tree[tuple(differ[0])]}, flat {flat[tuple(differ[0])]}"
    return tree


def _agree(got, want, what):
    """Every record of `got` has the reference's bits (a NaN for a NaN); the message names the first pixel that differs."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = fr.same_bits(got, want)
    bad = np.argwhere(~ok)
    print(f"{what}: {got.size} pixels, {int((want['sphere'] != MISS).sum())} reference hits, {len(bad)} records differ")
    assert ok.all(), f"{what}: {len(bad)} of {got.size} pixels differ, first compact pixel {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _check(ctx, ref, params, what):
    got = _tree_and_flat(ctx, params, what)
    _agree(got, ref.of(params), what)
    return got


def _params(w=fr.W, h=fr.H, spp=0, **kw):
    return m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, **kw)


# ---- 1. the fixture frame ----

FRAMES = {"spp 0": dict(spp=0), "spp 1": dict(spp=1), "spp 3": dict(spp=3), "sample_begin 5": dict(spp=1, sample_begin=5),
          "seed": dict(spp=1, seed=SEED)}


@BVH
@pytest.mark.parametrize("frame", list(FRAMES))
def test_fixture_frames_match_the_cpu_reference(ctx, frame, bvh):
    _set(ctx, fr.fixture_scene(), bvh)
    got = _check(ctx, fr.fixture(), _params(**FRAMES[frame]), f"{frame}, {bvh} tree")
    if frame == "seed":                                             # the seed reaches the kernel: the frame is not seed 0's
        assert not np.array_equal(_bytes(got), _bytes(ctx.render_features(_params(spp=1))))
    if frame == "sample_begin 5":
        assert not np.array_equal(_bytes(got), _bytes(ctx.render_features(_params(spp=1))))


@BVH
def test_a_lens_camera_carries_its_depth_of_field(ctx, bvh):
    _set(ctx, fr.fixture_scene(0.2), bvh)
    ref = fr.fixture(0.2)
    got = _check(ctx, ref, _params(spp=2), f"lens, spp 2, {bvh} tree")
    centre = _check(ctx, ref, _params(spp=0), f"lens, spp 0, {bvh} tree")
    pin = fr.fixture().frame(0)                                    # the centre ray ignores the lens: sphere and t are the pinhole camera's
    assert np.array_equal(centre["sphere"], pin["sphere"]) and np.array_equal(centre["t"].view(np.uint32), pin["t"].view(np.uint32))
    assert np.array_equal(got["sphere"], pin["sphere"])


# ---- 2. consistency with ray queries (the weaker check: the CPU reference is the judge) ----

def test_sphere_and_t_are_the_centre_rays_whatever_spp_and_equal_ray_queries(ctx):
    _set(ctx, fr.fixture_scene())
    f0 = ctx.render_features(_params(spp=0))
    for spp in (1, 3):
        f = ctx.render_features(_params(spp=spp))
        assert np.array_equal(f["sphere"], f0["sphere"]) and np.array_equal(f["t"].view(np.uint32), f0["t"].view(np.uint32)), spp
    cam = fr.fixture_camera()
    rays = np.concatenate([m.camera_pixel_ray(cam, fr.W, fr.H, x, y) for y in range(fr.H) for x in range(fr.W)])
    hits = ctx.trace_rays(rays).reshape(fr.H, fr.W)
    assert np.array_equal(hits["sphere"], f0["sphere"]) and np.array_equal(hits["t"].view(np.uint32), f0["t"].view(np.uint32))
    hit = f0["sphere"] != MISS                                      # at spp 0 the normal is the ray query's too
    assert np.array_equal(hits["normal"][hit].view(np.uint32), f0["normal"][hit].view(np.uint32))
    assert not _bytes(f0).reshape(fr.H, fr.W, 32)[~hit][:, :28].any()  # a miss: sphere = MISS and every other field 0


# ---- 3. partitions ----

@BVH
def test_row_bands_and_tile_partitions_are_rows_of_the_whole_frame(ctx, bvh):
    _set(ctx, fr.fixture_scene(), bvh)
    ref = fr.fixture()
    whole = ctx.render_features(_params(spp=1))
    band = _params(spp=1, row_begin=7, row_end=29)
    got = _check(ctx, ref, band, f"rows 7..29, {bvh} tree")
    assert got.shape == (22, fr.W) and np.array_equal(_bytes(got), _bytes(whole[7:29]))
    seen = []
    for part in range(3):
        p = _params(spp=1, tile_rows=4, n_parts=3, part=part)
        rows = [m.params_out_row_index(p, i) for i in range(m.params_out_rows(p))]
        got = _check(ctx, ref, p, f"tile_rows 4, part {part} of 3, {bvh} tree")
        assert np.array_equal(_bytes(got), _bytes(whole[rows])), part
        seen += rows
    assert sorted(seen) == list(range(fr.H))
    p = _params(spp=0, row_begin=8, row_end=40, tile_rows=4, n_parts=3, part=2)      # a band AND tiles: abs_row adds both
    rows = [m.params_out_row_index(p, i) for i in range(m.params_out_rows(p))]
    assert rows[0] == 16 and np.array_equal(_bytes(_check(ctx, ref, p, "band and tiles")), _bytes(ctx.render_features(_params(spp=0))[rows]))


# ---- 4. small and degenerate frames and worlds ----

@pytest.mark.parametrize("w, h", [(1, 1), (130, 1)])
def test_small_frames(ctx, w, h):
    arr, mats, tex = rq.field_world()
    cam = hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25)
    _set(ctx, hbm_worlds.scene_from_arrays(cam, arr, mats, tex))
    ref = fr.FeatureRef(arr, mats, tex, cam, w, h)
    for spp in (0, 2):
        got = _check(ctx, ref, _params(w, h, spp), f"{w} x {h}, spp {spp}")
    assert (got["sphere"] != MISS).any()


SMALL_W, SMALL_H = 9, 7


def _small_camera():
    return hbm_worlds.look(SMALL_W, SMALL_H, (0, 0, 2), (0, 0, -1), vfov=40)


def _small_world(name):
    """(SPHERE_DTYPE array, what the test asserts about it) for the 9 x 7 frames seen from (0, 0, 2) along -z."""
    if name == "single":
        return hbm_worlds.sphere_array([[0.5, -0.25, -5.0]], [1.25], [1])                      # the image texture
    if name == "copies":
        return hbm_worlds.sphere_array(np.tile([[0.3, 0.2, -4.0]], (1000, 1)), np.full(1000, 1.5), np.arange(1000) % 7)
    if name == "inside glass":                                      # the eye at the centre of a hollow glass sphere, another sphere outside
        return hbm_worlds.sphere_array([[0, 0, 2], [0, 0, 2], [0, 0, -3]], [1.0, -0.9, 1.0], [3, 3, 4])
    if name == "zero radius":
        # spheres of radius 0 ON the centre rays of pixels (4, 0) and (0, 3), whose directions have a zero component: the sphere test
        # finds a root by rounding, 1 / r = inf, and the zero component of point - centre makes inf x 0 = NaN in the normal
        cam = _small_camera()
        o, d = fr.centre_rays(cam, SMALL_W, SMALL_H, np.array([4, 0]), np.array([0, 3]))
        cen = (o.astype(np.float64) + d.astype(np.float64)).astype(f32)
        return hbm_worlds.sphere_array(np.concatenate([cen, [[0, 0, -30]]]), [0.0, 0.0, 3.0], [0, 3, 2])
    raise KeyError(name)


@BVH
@pytest.mark.parametrize("name", ["single", "copies", "inside glass", "zero radius"])
def test_small_worlds(ctx, name, bvh):
    arr = _small_world(name)
    mats, tex = hbm_worlds.field_materials()
    cam = _small_camera()
    _set(ctx, hbm_worlds.scene_from_arrays(cam, arr, mats, tex), bvh)
    ref = fr.FeatureRef(arr, mats, tex, cam, SMALL_W, SMALL_H)
    want = ref.frame(0)
    hit = want["sphere"] != MISS
    if name == "single":
        assert ctx.bvh_info()["plan"]["n_nodes"] == 0 and 0 < hit.sum() < hit.size
        assert len(np.unique(want["albedo"][hit], axis=0)) > 3       # image texels
    if name == "copies":
        assert hit.any() and (want["sphere"][hit] == 0).all()      # the lowest index wins among equals
    if name == "inside glass":
        assert hit.all() and (want["sphere"] == 1).all() and (want["albedo"] == 1).all()      # the inner surface, from inside
        centre = want["normal"][SMALL_H // 2, SMALL_W // 2]
        assert centre[2] > 0.99                                     # 1 / r < 0: the shading normal points AT the eye's side, inwards
    if name == "zero radius":
        assert want["sphere"][0, 4] == 0 and want["sphere"][3, 0] == 1
        assert np.isnan(want["normal"][0, 4]).any() and np.isnan(want["normal"][3, 0]).any()
    for spp in (0, 2):
        got = _check(ctx, ref, _params(SMALL_W, SMALL_H, spp), f"{name}, spp {spp}, {bvh} tree")
    if name == "zero radius":
        assert np.isnan(ctx.render_features(_params(SMALL_W, SMALL_H, 0))["normal"][0, 4]).any()


def test_the_empty_world_misses_everything(ctx):
    arr = _small_world("single")
    mats, tex = hbm_worlds.field_materials()
    _set(ctx, hbm_worlds.scene_from_arrays(_small_camera(), arr, mats, tex))
    ctx.set_spheres(arr[:0])
    for spp in (0, 3):
        got = _tree_and_flat(ctx, _params(SMALL_W, SMALL_H, spp), f"empty world, spp {spp}")
        assert (got["sphere"] == MISS).all() and not _bytes(got).reshape(-1, 32)[:, :28].any()


# ---- 5. the device call ----

def _device_features(ctx, torch, params, stream, offset=0, flat=False):
    """render_features_device into a torch buffer (4-byte aligned at `offset`) on a caller stream, a canary record behind the frame."""
    n = m.params_out_rows(params) * params.width
    with torch.cuda.stream(stream):
        d_out = torch.full((offset + 32 * n + 32 + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        ctx.render_features_device(params, d_out.data_ptr() + offset, 32 * n, flat=flat, stream=stream.cuda_stream)
        out = d_out.cpu().numpy()                                   # ordered after the kernel on the same stream
    assert (out[:offset] == 0x5A).all() and (out[offset + 32 * n:] == 0x5A).all(), "bytes around the records were written"
    return out[offset:offset + 32 * n].copy().view(FEATURE_DTYPE).reshape(-1, params.width)


def test_device_call_and_worlds_changed_on_the_device(ctx):
    import torch
    arr, mats, tex = hbm_worlds.rtiow_field(600)
    cam = hbm_worlds.look(fr.W, fr.H, (9, 2, 3), (0, 0.5, 0), vfov=30)
    _set(ctx, hbm_worlds.scene_from_arrays(cam, arr, mats, tex), "device")
    stream = torch.cuda.Stream(device="cuda:0")
    for spp, offset, flat in ((0, 0, False), (1, 4, False), (1, 0, True), (3, 12, False)):
        p = _params(spp=spp)
        got = _device_features(ctx, torch, p, stream, offset, flat)
        assert ctx.last_kernel() == ("feature_frame_kernel<false>" if flat else "feature_frame_kernel<true>")
        assert np.array_equal(_bytes(got), _bytes(ctx.render_features(p, flat=flat))), (spp, offset, flat)
    p = _params(spp=1, tile_rows=4, n_parts=3, part=1)               # a partition, with the canary behind ITS last record
    _agree(_device_features(ctx, torch, p, stream, 4), fr.FeatureRef(arr, mats, tex, cam, fr.W, fr.H).of(p), "device call, part 1 of 3")
    # spheres moved from a device tensor: the refitted tree shows the moved world
    rng = np.random.default_rng(8)
    moved = arr.copy()
    first, count = 100, 300
    moved["center"][first:first + count, :3] += rng.normal(0, 1.0, (count, 3)).astype(f32)
    moved["radius"][first:first + count] *= rng.uniform(0.5, 3.0, count).astype(f32)
    d_moved = torch.from_numpy(_bytes(moved[first:first + count]).copy()).to("cuda:0")
    before = ctx.render_features(_params(spp=1))
    ctx.update_spheres_device(first, count, d_moved.data_ptr())
    ref = fr.FeatureRef(moved, mats, tex, cam, fr.W, fr.H)
    got = _check(ctx, ref, _params(spp=1), "after update_spheres_device")
    assert not np.array_equal(_bytes(got), _bytes(before)), "the move changes the frame"
    _agree(_device_features(ctx, torch, _params(spp=1), stream), ref.of(_params(spp=1)), "device call after update_spheres_device")
    # another count, from a device tensor
    fewer = np.concatenate([moved[:5], moved[250:550]])
    d_fewer = torch.from_numpy(_bytes(fewer).copy()).to("cuda:0")
    ctx.set_spheres_device(len(fewer), d_fewer.data_ptr())
    ref = fr.FeatureRef(fewer, mats, tex, cam, fr.W, fr.H)
    _check(ctx, ref, _params(spp=1), "after set_spheres_device")
    _agree(_device_features(ctx, torch, _params(spp=1), stream, 4), ref.of(_params(spp=1)), "device call after set_spheres_device")


# ---- 6. errors, and what a feature frame leaves alone ----

def _lds_scene():
    scene, cam = m.scenes.three_spheres()
    return m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))


def test_every_error_code_and_a_refused_call_queues_nothing(ctx):
    lib = m.lib()
    out = np.zeros((fr.H + 1, fr.W), FEATURE_DTYPE)
    po, n = C.c_void_p(out.ctypes.data), fr.H * fr.W * 32

    def both(params, flags, o, nbytes):
        pp = C.byref(params) if params is not None else None
        a = lib.mirt_ctx_render_features(ctx._h, pp, flags, o, nbytes)
        b = lib.mirt_ctx_render_features_device(ctx._h, pp, flags, o, nbytes, None)
        assert a == b, (a, b)
        return a

    ctx.set_scene(_lds_scene())                                     # an LDS scene: no table and no tree to look at
    assert both(_params(64, 48), 0, po, n) == _abi.MIRT_ERR_NO_SCENE and b"MIRT_SCENE_HBM" in lib.mirt_last_error()
    with pytest.raises(m.MirtError) as e:
        ctx.render_features(_params(64, 48))
    assert e.value.status == _abi.MIRT_ERR_NO_SCENE
    _set(ctx, fr.fixture_scene())
    img = ctx.render(_params(spp=2))
    kernel = ctx.last_kernel()
    ok = _params()
    assert both(None, 0, po, n) == _abi.MIRT_ERR_NULL_POINTER and both(ok, 0, None, n) == _abi.MIRT_ERR_NULL_POINTER
    for bad in (2, 3, 1 << 31, 0xFFFFFFFE):
        assert both(ok, bad, po, n) == _abi.MIRT_ERR_BAD_MODE
    assert both(_params(0, fr.H), 0, po, n) == _abi.MIRT_ERR_VIEWPORT_SIZE == lib.mirt_ctx_render(ctx._h, C.byref(_params(0, fr.H, 1)), po, n)
    assert both(_params(fr.W, 0), 0, po, n) == _abi.MIRT_ERR_VIEWPORT_SIZE
    for rows in (dict(row_begin=30, row_end=20), dict(row_end=fr.H + 1), dict(tile_rows=4, n_parts=3, part=3)):
        assert both(_params(**rows), 0, po, n) == _abi.MIRT_ERR_BAD_ROWS == lib.mirt_ctx_render(ctx._h, C.byref(_params(spp=1, **rows)), po, n), rows
    assert both(_params(spp=_abi.MIRT_MAX_SPP_PER_CALL + 1), 0, po, n) == _abi.MIRT_ERR_SPP_RANGE
    assert both(_params(spp=2, sample_begin=0xFFFFFFFE), 0, po, n) == _abi.MIRT_ERR_SPP_RANGE
    assert both(_params(spp=2, frame_spp=2), 0, po, n) == _abi.MIRT_ERR_FRAME_SPP
    assert both(_params(spp=0, frame_spp=1), 0, po, n) == _abi.MIRT_ERR_FRAME_SPP
    assert both(ok, 0, po, n - 1) == _abi.MIRT_ERR_OUT_BUFFER and both(ok, 0, po, 0) == _abi.MIRT_ERR_OUT_BUFFER
    assert both(_params(row_begin=7, row_end=29), 0, po, 22 * fr.W * 32 - 1) == _abi.MIRT_ERR_OUT_BUFFER
    assert ctx.last_kernel() == kernel, "a refused call queues nothing"
    assert not _bytes(out).any()
    # mode, num_bounces, flags and frame_begin are not read
    plain = ctx.render_features(_params(spp=1))
    odd = m.make_params(fr.W, fr.H, 1, mode=77, num_bounces=0, flags=0xFFFFFFFF, frame_begin=9)
    assert np.array_equal(_bytes(ctx.render_features(odd)), _bytes(plain))
    assert np.array_equal(ctx.render(_params(spp=2)), img)
    # scenes whose tables a path-traced render refuses: the same answer here (ray queries do not read materials; this call does)
    arr, mats, tex = rq.field_world()
    bad_index = arr[:50].copy()
    bad_index["material_idx"][17] = len(mats)
    ctx.set_scene(hbm_worlds.scene_from_arrays(fr.fixture_camera(), bad_index, mats, tex), hbm=True)
    assert both(ok, 0, po, n) == _abi.MIRT_ERR_MATERIAL_INDEX == lib.mirt_ctx_render(ctx._h, C.byref(_params(spp=1)), po, n)
    assert len(ctx.trace_rays(m.camera_pixel_ray(fr.fixture_camera(), fr.W, fr.H, 3, 3))) == 1
    ctx.set_spheres(bad_index)                                      # the device's own check of a new table answers the same
    assert both(ok, 0, po, n) == _abi.MIRT_ERR_MATERIAL_INDEX
    past = [_abi.MirtMaterial.from_buffer_copy(bytes(x)) for x in mats]
    past[0].desc1.offset = len(np.asarray(tex).reshape(-1, 3))
    ctx.set_scene(hbm_worlds.scene_from_arrays(fr.fixture_camera(), arr[:50], past, tex), hbm=True)
    assert both(ok, 0, po, n) == _abi.MIRT_ERR_TEXEL_RANGE == lib.mirt_ctx_render(ctx._h, C.byref(_params(spp=1)), po, n)
    assert not _bytes(out).any()


def test_a_feature_frame_leaves_renders_statistics_and_sums_alone(ctx):
    _set(ctx, fr.fixture_scene())
    p = m.make_params(fr.W, fr.H, 4, mode=m.MIRT_MODE_PT, num_bounces=4)
    img = ctx.render(p)
    kernel = ctx.last_kernel()
    ctx.accum_reset(p)
    ctx.accum_add(p)
    sums = ctx.accum_read(p)
    before = ctx.stats()
    got = ctx.render_features(_params(spp=2))
    assert ctx.last_kernel() == "feature_frame_kernel<true>" != kernel
    assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p), sums)
    after = ctx.stats()
    assert after["launches"] == 0 and after["kernel_ms_total"] == 0                     # a feature frame is no render launch
    assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
    st = ctx.trace_stats()
    assert st["kernel_ms"] > 0 and not any(v for k, v in st.items() if k != "kernel_ms")   # the trace call's event pair, no counters
    assert np.array_equal(ctx.render(p), img), "a render after the feature call gives the bytes it gave before"
    _agree(got, fr.fixture().of(_params(spp=2)), "a feature frame between renders")
    ctx.set_timing(False)
    ctx.render_features(_params())
    assert ctx.trace_stats()["kernel_ms"] == 0.0
    ctx.set_timing(True)
    import torch
    d_out = torch.zeros(fr.H * fr.W * 32, dtype=torch.uint8, device="cuda:0")
    ctx.render_features_device(_params(), d_out.data_ptr(), d_out.numel())         # the context's own stream: synchronize waits for it
    ctx.synchronize()
    assert ctx.trace_stats()["kernel_ms"] > 0.0
    assert np.array_equal(d_out.cpu().numpy(), _bytes(ctx.render_features(_params())).ravel())


# ---- 7. Layer.features and Raytracer.features ----

def _planes_agree(planes, want, what):
    got = np.zeros(want.shape, FEATURE_DTYPE)
    for k in ("albedo", "normal", "t", "sphere"):
        assert planes[k].shape == want[k].shape, (what, k)
        got[k] = planes[k]
    _agree(got, want, what)


def test_layer_and_raytracer_features():
    w, h = 67, 45
    scene = m.Layer.scene()                                         # six spheres, two image textures: a world that lives in LDS
    cam = m.FlyCameraController.default().renderer_camera()
    rp = m.RenderParams(camera=cam, viewport_size=(w, h))
    arr = hbm_worlds.sphere_array([s.center for s in scene.spheres], [s.radius for s in scene.spheres], [s.material_idx for s in scene.spheres])
    layer = m.Layer.new([w, h], rp, scene=scene)
    layer.set_global_data()
    try:
        layer.set_data(rp)
        assert not layer._hbm
        rgba = layer.register_texture().copy()
        ref = fr.FeatureRef(arr, layer.material_data, layer.global_texture_data, layer.camera.c, w, h)
        planes = layer.features()
        assert layer._hbm and layer._ctx.last_kernel() == "feature_frame_kernel<true>"
        assert planes["albedo"].shape == (h, w, 3) and planes["sphere"].dtype == np.uint32
        _planes_agree(planes, ref.frame(0), "Layer.features()")
        assert (planes["sphere"] == MISS).any() and len(np.unique(planes["sphere"])) >= 4
        hit = layer.pick(30, 30)                                    # pick's ray is float64 on the host: the sphere agrees, not the bits
        assert (hit["sphere"] if hit else MISS) == planes["sphere"][30, 30]
        layer.set_data(rp)
        assert np.array_equal(layer.register_texture(), rgba)
        with pytest.raises(ValueError):
            layer.features(-1)
    finally:
        layer.close()
    rt = m.Raytracer(scene, rp)
    try:
        ref = fr.FeatureRef(arr, rt.material_data, rt.global_texture_data, rt.camera.c, w, h)
        _planes_agree(rt.features(spp=2), ref.frame(2), "Raytracer.features(spp=2)")
        _planes_agree(rt.features(), ref.frame(rp.sampling.num_samples_per_pixel), "Raytracer.features()")
        _planes_agree(rt.features(spp=1, seed=SEED), ref.frame(1, 0, SEED), "Raytracer.features(spp=1, seed)")
    finally:
        rt.close()
