"""MIRT_QUERY_LDS on the device: ray queries, feature frames and radiance queries on a scene that stays in LDS
(trace_rays_lds_kernel<GRID,ANY,COUNT>, feature_frame_lds_kernel<GRID>, radiance_rays_lds_kernel<HOSEK,GRID>) must return the bytes the
same call returns on a second context that holds the same world as a MIRT_SCENE_HBM scene with a device-built tree -- every record, bit
for bit, a NaN for a NaN -- and, where a CPU reference exists (tests/ray_query_ref.py, feature_ref.py, radiance_ref.py), that reference's.
Without the flag every call here answers MIRT_ERR_NO_SCENE, and a library that does not know the flag MIRT_ERR_BAD_MODE.  The worlds and
ray sets are those of tests/query_lds_worlds.py (their preconditions: tests/test_query_lds_abi.py); the references are computed once."""
import ctypes as C

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from weekend_raytracer_wgpu_amd.context import FEATURE_DTYPE, RADIANCE_DTYPE, RAY_HIT_DTYPE
import feature_ref as fr
import hbm_worlds
import query_lds_worlds as qw
import radiance_ref as rr
import ray_query_ref as rq

pytestmark = pytest.mark.gpu

FLAT, ANY, COUNT, SORT, LDS = m.MIRT_RAYS_FLAT, m.MIRT_RAYS_ANY_HIT, m.MIRT_RAYS_COUNT, m.MIRT_RAYS_SORT, m.MIRT_QUERY_LDS
TF = ("false", "true")
f32 = np.float32
ALL = tuple(range(rr.N_RAYS))
SUBSET = (0, 1, 5, 6, rr.INSIDE_HERO, rr.MISSES_ALL, 30, 31)
FOUR = rr.BOUNCE_RAYS


class Pair:
    """Two contexts holding one world: `lds` in LDS, `hbm` as MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE."""
    def __init__(self):
        self.lds, self.hbm, self.key = m.Context(0), m.Context(0), None

    def use(self, key, scene=None, bvh="device"):
        if self.key != (key, bvh):
            sd = scene if scene is not None else qw.world(key)
            self.lds.set_scene(sd)
            self.hbm.set_scene(sd, hbm=True, bvh=bvh)
            assert self.hbm.bvh_info()["built_on_device"] == (bvh == "device")
            with pytest.raises(m.MirtError) as e:                   # the first context's scene lives in LDS: no tree
                self.lds.bvh_info()
            assert e.value.status == _abi.MIRT_ERR_NO_SCENE
            self.key = (key, bvh)
        return self.lds, self.hbm

    def close(self):
        self.lds.close()
        self.hbm.close()


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what, same_bits=rq.same_bits):
    ok = same_bits(got, want)
    bad = np.argwhere(~ok)
    assert ok.all(), f"{what}: {len(bad)} of {got.size} records differ, first {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _layouts(name):
    """(flat bit, the GRID template argument) of the layouts a world has in LDS."""
    _, grid, flat = qw.WORLDS[name]
    return ([(False, True)] if grid else []) + ([(True, False)] if flat else []) + ([(False, False)] if not grid else [])


# ---- 1. ray queries ----

@pytest.mark.parametrize("name", [n for n in qw.WORLDS if n != "radiance sky"])        # (ray queries read no sky)
def test_ray_queries_return_the_twins_bytes(pair, name):
    lds, hbm = pair.use(name)
    for key, (o, d, defined) in qw.ray_sets(name).items():
        for t_max in qw.T_MAXES:
            rays = rq.rays_of(o, d, t_max)
            for flags in (0, ANY):
                twin = hbm.trace_rays(rays, flags)
                what = f"{name}, rays '{key}', t_max {t_max}, flags {flags:#x}"
                if flags == 0:
                    _same(twin[defined], qw.reference(name, key, t_max), what + " (the twin against the CPU reference)")
                for flat, grid in _layouts(name):
                    got = lds.trace_rays(rays, flags | (FLAT if flat else 0), lds=True)
                    assert lds.last_kernel() == f"trace_rays_lds_kernel<{TF[grid]},{TF[flags == ANY]},false>", what
                    _same(got, twin, what + f", grid {grid}")
                if flags == 0 and t_max == np.inf:
                    hit = got["sphere"] != rq.MISS
                    print(f"{name}, rays '{key}': {len(o)} rays, {int(hit.sum())} hits without a bound, {int((got['t'][hit] > 1000.0).sum())} of them beyond t = 1000")
                    assert key != "long t" or name not in ("field 484", "main.rs", "fixture") or (got["t"][hit] > 1000.0).sum() >= 32, what
    if not qw.WORLDS[name][2]:                                      # grid only: the _FLAT bit has no layout
        with pytest.raises(m.MirtError) as e:
            lds.trace_rays(rays, FLAT, lds=True)
        assert e.value.status == _abi.MIRT_ERR_SCENE_TOO_LARGE


def test_the_host_built_tree_is_the_same_twin(pair):
    lds, hbm = pair.use("field 484", bvh="host")
    o, d = qw.aimed_rays("field 484")
    rays = rq.rays_of(o, d, np.inf)
    twin = hbm.trace_rays(rays)
    for flat in (False, True):
        _same(lds.trace_rays(rays, FLAT if flat else 0, lds=True), twin, f"host-built twin, flat {flat}")


@pytest.mark.parametrize("name", ["field 484", "main.rs", "far origins"])
def test_counters(pair, name):
    lds, hbm = pair.use(name)
    o = np.concatenate([s[0] for s in qw.ray_sets(name).values()])
    d = np.concatenate([s[1] for s in qw.ray_sets(name).values()])
    rays = rq.rays_of(o, d, np.inf)
    n, n_spheres = len(rays), len(qw.spheres(name)[0])
    for flags in (0, ANY):
        plain = hbm.trace_rays(rays, flags | FLAT)
        assert np.array_equal(_bytes(hbm.trace_rays(rays, flags | FLAT | COUNT)), _bytes(plain))
        twin = hbm.trace_stats()
        assert twin["rays"] == n and (flags == ANY or twin["sphere_tests"] == n * n_spheres)
        for flat, grid in _layouts(name):
            got = lds.trace_rays(rays, flags | COUNT | (FLAT if flat else 0), lds=True)
            assert lds.last_kernel() == f"trace_rays_lds_kernel<{TF[grid]},{TF[flags == ANY]},true>"
            assert np.array_equal(_bytes(got), _bytes(plain))
            st = lds.trace_stats()
            print(name, f"flags {flags:#x} grid {grid}", st, "twin", twin)
            assert st["rays"] == twin["rays"] and st["hits"] == twin["hits"] and st["kernel_ms"] > 0.0
            if not grid:
                assert all(st[k] == twin[k] for k in ("sphere_tests", "roots")) and st["nodes"] == 0 and st["wave_nodes"] == 0
            else:
                assert 0 < st["sphere_tests"] < twin["sphere_tests"] or flags == ANY
                assert st["hits"] <= st["roots"] <= 2 * st["sphere_tests"]
                assert 0 < st["wave_nodes"] <= st["nodes"] <= 64 * st["wave_nodes"]
            lds.trace_rays(rays[:64], flags | (FLAT if flat else 0), lds=True)
            assert not any(v for k, v in lds.trace_stats().items() if k != "kernel_ms"), "no counters without MIRT_RAYS_COUNT"


def test_batch_sizes_and_the_record_behind_the_last(pair):
    lds, hbm = pair.use("field 484")
    o, d = qw.aimed_rays("field 484")
    rays = rq.rays_of(o, d, np.inf)
    twin = hbm.trace_rays(rays)
    lib = m.lib()
    for flat in (0, FLAT):
        for n in (1, 63, 64, 65, 257):
            hits = np.zeros(n + 1, RAY_HIT_DTYPE)
            _bytes(hits)[:] = 0xA5                                  # the canary: record n must stay as it is
            rc = lib.mirt_ctx_trace_rays(lds._h, C.c_void_p(rays.ctypes.data), n, LDS | flat, C.c_void_p(hits.ctypes.data))
            assert rc == 0, lib.mirt_last_error()
            assert np.array_equal(_bytes(hits[:n]), _bytes(twin[:n])), (flat, n)
            assert (_bytes(hits[n:]) == 0xA5).all(), f"n = {n}: the record behind the last was written"


def test_one_block_strides_over_the_units(monkeypatch, pair):
    """MIRT_QUERY_LDS_BLOCKS=1: four waves in all.  769 rays are three full units per wave and one lane in a thirteenth unit; a 67 x 45
    frame is 48 units, the last one 7 pixels; 8 radiance rays leave three waves of the live block without a unit."""
    monkeypatch.setenv("MIRT_QUERY_LDS_BLOCKS", "1")                # read when a context is created
    _, hbm = pair.use("field 484")
    o, d = qw.aimed_rays("field 484")
    rays = rq.rays_of(np.concatenate([o, o[:257]]), np.concatenate([d, d[:257]]), np.inf)
    assert len(rays) == 769
    rad_rays = m.make_radiance_rays(o[:8], d[:8], np.arange(8))
    many = m.make_radiance_rays(rays["origin"], rays["direction"], np.arange(769))
    p = m.make_params(67, 45, 1, mode=m.MIRT_MODE_PT)
    with m.Context(0) as own:
        own.set_scene(qw.world("field 484"))
        for flat in (False, True):
            assert np.array_equal(_bytes(own.trace_rays(rays, FLAT if flat else 0, lds=True)), _bytes(hbm.trace_rays(rays))), flat
            assert np.array_equal(_bytes(own.trace_rays(rays, ANY | (FLAT if flat else 0), lds=True)), _bytes(hbm.trace_rays(rays, ANY))), flat
            assert np.array_equal(_bytes(own.render_features(p, flat=flat, lds=True)), _bytes(hbm.render_features(p))), flat
            assert np.array_equal(_bytes(own.trace_radiance(rad_rays, 2, flat=flat, lds=True)), _bytes(hbm.trace_radiance(rad_rays, 2))), flat
            assert np.array_equal(_bytes(own.trace_radiance(many, 1, flat=flat, lds=True)), _bytes(hbm.trace_radiance(many, 1))), flat


def test_the_sort_hint_is_ignored_and_the_order_stays(pair):
    o, d = qw.aimed_rays("field 484")
    rays = rq.rays_of(o, d, np.inf)
    with m.Context(0) as own:
        own.set_scene(qw.world("field 484"), hbm=True)
        first = own.trace_rays(rays[:100], sort=True)
        assert own.last_kernel().startswith("trace_rays_sorted_kernel<")
        order = own.trace_order()
        assert sorted(order.tolist()) == list(range(100))
        own.set_scene(qw.world("field 484"))                        # the same world, now in LDS
        lib = m.lib()
        raw = np.zeros(100, np.uint32)
        before = (lib.mirt_ctx_trace_order_read(own._h, C.c_void_p(raw.ctypes.data), 100), raw.copy())
        for flags in (SORT, SORT | FLAT, SORT | ANY):
            got = own.trace_rays(rays, flags & ~SORT, sort=True, lds=True)
            assert own.last_kernel() == f"trace_rays_lds_kernel<{TF[not flags & FLAT]},{TF[bool(flags & ANY)]},false>"
            if not flags & ANY:
                assert np.array_equal(_bytes(got[:100]), _bytes(first))
                assert np.array_equal(_bytes(got), _bytes(own.trace_rays(rays, flags & FLAT, lds=True)))
        rad_rays = m.make_radiance_rays(o[:64], d[:64], np.arange(64))
        own.trace_radiance(rad_rays, 1, sort=True, pool=True, lds=True)
        raw[:] = 0
        after = (lib.mirt_ctx_trace_order_read(own._h, C.c_void_p(raw.ctypes.data), 100), raw.copy())
        assert before[0] == after[0] and np.array_equal(before[1], after[1]), "the order of the last launch that really sorted"
        if before[0] == 0:
            assert np.array_equal(own.trace_order(), order)


def test_device_pointers_on_a_callers_stream(pair):
    import torch
    lds, hbm = pair.use("field 484")
    o, d = qw.aimed_rays("field 484")
    rays = rq.rays_of(o, d, np.inf)
    n = len(rays)
    stream = torch.cuda.Stream(device="cuda:0")
    rad_rays = m.make_radiance_rays(o, d, np.arange(n))
    p = m.make_params(67, 5, 1, mode=m.MIRT_MODE_PT)
    with torch.cuda.stream(stream):
        d_in = torch.from_numpy(_bytes(rays).copy()).to("cuda:0")
        d_rad = torch.from_numpy(_bytes(rad_rays).copy()).to("cuda:0")
        for flat in (False, True):
            d_out = torch.full((32 * n + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
            lds.trace_rays_device(d_in.data_ptr(), n, d_out.data_ptr() + 4, FLAT if flat else 0, stream=stream.cuda_stream, lds=True)
            out = d_out.cpu().numpy()
            assert np.array_equal(out[4:4 + 32 * n], _bytes(hbm.trace_rays(rays))) and (out[:4] == 0x5A).all() and (out[4 + 32 * n:] == 0x5A).all()
            d_out.fill_(0x5A)
            lds.trace_radiance_device(d_rad.data_ptr(), n, d_out.data_ptr() + 4, 2, stream=stream.cuda_stream, flat=flat, lds=True)
            out = d_out.cpu().numpy()
            assert np.array_equal(out[4:4 + 32 * n], _bytes(hbm.trace_radiance(rad_rays, 2))) and (out[:4] == 0x5A).all() and (out[4 + 32 * n:] == 0x5A).all()
            d_out.fill_(0x5A)
            lds.render_features_device(p, d_out.data_ptr() + 4, 67 * 5 * 32, flat=flat, stream=stream.cuda_stream, lds=True)
            out = d_out.cpu().numpy()
            assert np.array_equal(out[4:4 + 32 * 335], _bytes(hbm.render_features(p)).reshape(-1)) and (out[:4] == 0x5A).all() and (out[4 + 32 * 335:] == 0x5A).all()
    assert lds.trace_stats()["kernel_ms"] > 0.0


# ---- 2. feature frames ----

def _feature_case(w, h, aperture):
    arr, mats, tex = hbm_worlds.rtiow_field(484)
    cam = hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25, aperture=aperture)
    return fr.FeatureRef(arr, mats, tex, cam, w, h), hbm_worlds.scene_from_arrays(cam, arr, mats, tex)


@pytest.mark.parametrize("w,h", [(48, 32), (67, 5)])
def test_feature_frames(pair, w, h):
    """The field of 484 spheres -- image texture, checkerboard, glass, a missing material -- through a lens, in both layouts."""
    ref, scene = _feature_case(w, h, 0.1)
    lds, hbm = pair.use(f"features {w}x{h}", scene)
    seen = set()
    for kw in (dict(spp=0), dict(spp=1), dict(spp=4), dict(spp=1, row_begin=h // 4, row_end=h - 1), dict(spp=1, tile_rows=2, n_parts=3, part=1)):
        p = m.make_params(w, h, mode=m.MIRT_MODE_PT, **kw)
        twin, want = hbm.render_features(p), ref.of(p)
        _same(twin, want, f"{w} x {h} {kw}: the twin against the CPU reference", fr.same_bits)
        for flat in (False, True):
            got = lds.render_features(p, flat=flat, lds=True)
            assert lds.last_kernel() == f"feature_frame_lds_kernel<{TF[not flat]}>" and got.dtype == FEATURE_DTYPE and got.shape == twin.shape
            _same(got, twin, f"{w} x {h} {kw}, flat {flat}", fr.same_bits)
        hit = want["sphere"] != fr.MISS
        seen |= set(ref.arr["material_idx"][want["sphere"][hit]].tolist())
    mats = hbm_worlds.field_materials()[0]
    ids = {int(_abi.MirtMaterial.from_buffer_copy(bytes(mats[i])).id) for i in seen}
    assert fr.IMAGE_MATERIAL in seen and 3 in ids, f"the frames show an image texture and a checkerboard: materials {seen}, routines {ids}"


def test_feature_frames_of_the_fixture(pair):
    """rtiow_field(3000) at 67 x 45: an 84 KB blob and 96 KB of flat tables, one block per CU either way."""
    lds, hbm = pair.use("fixture")
    for spp in (0, 1):
        p = m.make_params(fr.W, fr.H, spp, mode=m.MIRT_MODE_PT)
        want = fr.fixture().of(p)
        for flat in (False, True):
            _same(lds.render_features(p, flat=flat, lds=True), want, f"fixture, spp {spp}, flat {flat}", fr.same_bits)
        _same(hbm.render_features(p), want, f"fixture, spp {spp}: the twin", fr.same_bits)


# ---- 3. radiance ----

def _agree(got, want, what):
    assert got.dtype == want.dtype == RADIANCE_DTYPE and got.shape == want.shape
    bad = np.nonzero((_bytes(got).reshape(-1, 32) != _bytes(want).reshape(-1, 32)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _radiance(lds, rays, spp, what, hosek=False, **kw):
    """The grid build's records, after checking that the flat layout returns the same bytes."""
    grid = lds.trace_radiance(rays, spp, hosek=hosek, lds=True, **kw)
    assert lds.last_kernel() == f"radiance_rays_lds_kernel<{TF[hosek]},true>", what
    flat = lds.trace_radiance(rays, spp, hosek=hosek, flat=True, lds=True, **kw)
    assert lds.last_kernel() == f"radiance_rays_lds_kernel<{TF[hosek]},false>", what
    _agree(flat, grid, what + ": flat against grid")
    return grid


def test_radiance_equals_the_oracle_and_the_twin(pair):
    lds, hbm = pair.use("radiance")
    rays = rr.rays_and_streams(ALL)
    got = _radiance(lds, rays, 4, "32 rays x 8 streams")
    _agree(got, rr.oracle_records(ALL), "32 rays x 8 streams against the oracle")
    _agree(got, hbm.trace_radiance(rays, 4), "32 rays x 8 streams against the twin")
    sub = rr.rays_and_streams(SUBSET)
    later = _radiance(lds, sub, 4, "sample_begin 4", sample_begin=4)
    _agree(later, rr.oracle_records(SUBSET, sample_begin=4), "sample_begin 4 against the oracle")
    _agree(later, hbm.trace_radiance(sub, 4, sample_begin=4), "sample_begin 4 against the twin")
    # MIRT_RADIANCE_ACCUMULATE twice against one call of 8
    whole = _radiance(lds, sub, 8, "spp 8")
    _agree(whole, rr.oracle_records(SUBSET, spp=8), "spp 8 against the oracle")
    for flat in (False, True):
        part = lds.trace_radiance(sub, 4, flat=flat, lds=True)
        _agree(part, rr.oracle_records(SUBSET), "the first four")
        back = lds.trace_radiance(sub, 4, sample_begin=4, flat=flat, into=part, lds=True)
        assert back is part and (part["samples"] == 8).all()
        _agree(part, whole, f"4 + 4 accumulated, flat {flat}")
    # bounces
    four = rr.rays_and_streams(FOUR)
    for nb in (1, 8):
        got = _radiance(lds, four, 4, f"{nb} bounces", num_bounces=nb)
        _agree(got, rr.oracle_records(FOUR, num_bounces=nb), f"{nb} bounces against the oracle")
        _agree(got, hbm.trace_radiance(four, 4, num_bounces=nb), f"{nb} bounces against the twin")
    # the schedule hints: the same bytes from the unpooled LDS kernel
    for kw in (dict(pool=True), dict(sort=True), dict(pool=True, sort=True)):
        _agree(_radiance(lds, sub, 4, f"{kw}", **kw), rr.oracle_records(SUBSET), f"{kw}")


def test_radiance_under_the_hosek_sky_in_both_layouts(pair):
    lds, hbm = pair.use("radiance sky")
    sub = rr.rays_and_streams(SUBSET)
    got = _radiance(lds, sub, 4, "Hosek sky", hosek=True)
    _agree(got, rr.oracle_records(SUBSET, hosek=True), "Hosek sky against the oracle")
    _agree(got, hbm.trace_radiance(sub, 4, hosek=True), "Hosek sky against the twin")
    plain = _radiance(lds, sub, 4, "a scene with a blob, queried without the flag")
    _agree(plain, rr.oracle_records(SUBSET), "a scene with a blob, queried without the flag")
    assert not np.array_equal(_bytes(plain), _bytes(got))


def test_radiance_on_the_grid_only_world(pair):
    lds, hbm = pair.use("field 4000")
    o, d = qw.aimed_rays("field 4000")
    rays = m.make_radiance_rays(o[:256], d[:256], np.arange(256))
    got = lds.trace_radiance(rays, 2, lds=True)
    assert lds.last_kernel() == "radiance_rays_lds_kernel<false,true>"
    _agree(got, hbm.trace_radiance(rays, 2), "4000 spheres, grid")
    p = m.make_params(48, 32, 1, mode=m.MIRT_MODE_PT)
    _same(lds.render_features(p, lds=True), hbm.render_features(p), "4000 spheres, a feature frame", fr.same_bits)
    for call in (lambda: lds.trace_radiance(rays, 2, flat=True, lds=True), lambda: lds.render_features(p, flat=True, lds=True)):
        kernel = lds.last_kernel()
        with pytest.raises(m.MirtError) as e:
            call()
        assert e.value.status == _abi.MIRT_ERR_SCENE_TOO_LARGE and lds.last_kernel() == kernel


# ---- 4. across the families ----

def test_an_hbm_scene_ignores_the_flag(pair):
    _, hbm = pair.use("field 484")
    o, d = qw.aimed_rays("field 484")
    rays, rad_rays = rq.rays_of(o, d, np.inf), m.make_radiance_rays(o, d, np.arange(len(o)))
    p = m.make_params(48, 32, 1, mode=m.MIRT_MODE_PT)
    calls = [lambda **kw: hbm.trace_rays(rays, **kw), lambda **kw: hbm.trace_rays(rays, FLAT | ANY, **kw), lambda **kw: hbm.trace_rays(rays, sort=True, **kw),
             lambda **kw: hbm.render_features(p, **kw), lambda **kw: hbm.render_features(p, flat=True, **kw),
             lambda **kw: hbm.trace_radiance(rad_rays, 2, **kw), lambda **kw: hbm.trace_radiance(rad_rays, 2, pool=True, **kw),
             lambda **kw: hbm.trace_radiance(rad_rays, 2, flat=True, sort=True, **kw)]
    for call in calls:
        plain = call()
        kernel = hbm.last_kernel()
        flagged = call(lds=True)
        assert hbm.last_kernel() == kernel and "_lds_" not in kernel and np.array_equal(_bytes(plain), _bytes(flagged)), kernel


def _lds_three():
    scene, cam = m.scenes.three_spheres()
    return m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))


def test_every_refusal_keeps_its_code_with_the_flag_set():
    """The refusals of tests/test_gpu_trace_rays.py, test_gpu_features.py and test_gpu_trace_radiance.py, on a scene in LDS with the flag."""
    lib = m.lib()
    E = _abi
    with m.Context(0) as ctx:
        o, d = qw.aimed_rays("radiance")
        rays, hits = rq.rays_of(o[:100], d[:100]), np.zeros(100, RAY_HIT_DTYPE)
        rad_rays, rad_out = rr.rays_and_streams(SUBSET), np.zeros(len(SUBSET) * rr.N_STREAMS, RADIANCE_DTYPE)
        feat = np.zeros((49, 64), FEATURE_DTYPE)
        for a in (hits, rad_out, feat):
            _bytes(a)[:] = 0xA5
        pr, ph = C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data)
        qr, qo, qn = C.c_void_p(rad_rays.ctypes.data), C.c_void_p(rad_out.ctypes.data), len(rad_rays)
        po, pn = C.c_void_p(feat.ctypes.data), 48 * 64 * 32
        P = _abi.MirtRadianceParams
        params = lambda w=64, h=48, spp=0, **kw: m.make_params(w, h, spp, mode=m.MIRT_MODE_PT, **kw)

        def trace(flags, a=pr, b=ph, n=100):
            r = (lib.mirt_ctx_trace_rays(ctx._h, a, n, flags, b), lib.mirt_ctx_trace_rays_device(ctx._h, a, n, flags, b, None))
            assert r[0] == r[1], r
            return r[0]

        def features(p, flags, out=po, nbytes=pn):
            pp = C.byref(p) if p is not None else None
            r = (lib.mirt_ctx_render_features(ctx._h, pp, flags, out, nbytes), lib.mirt_ctx_render_features_device(ctx._h, pp, flags, out, nbytes, None))
            assert r[0] == r[1], r
            return r[0]

        def radiance(p, a=qr, b=qo, n=qn):
            pp = C.byref(p) if p is not None else None
            r = (lib.mirt_ctx_trace_radiance(ctx._h, a, n, pp, b), lib.mirt_ctx_trace_radiance_device(ctx._h, a, n, pp, b, None))
            assert r[0] == r[1], r
            return r[0]

        # no scene at all, flag or not
        assert trace(LDS) == features(params(), LDS) == radiance(P(4, 0, 8, LDS, 0)) == E.MIRT_ERR_NO_SCENE
        ctx.set_scene(qw.world("radiance"))
        img = ctx.render(params(spp=2))
        kernel = ctx.last_kernel()
        # a scene in LDS without the flag: as ever
        assert trace(0) == features(params(), 0) == radiance(P(4, 0, 8, 0, 0)) == E.MIRT_ERR_NO_SCENE and b"MIRT_QUERY_LDS" in lib.mirt_last_error()
        # unknown bits beside the flag (bits 3 and 5 stay unassigned)
        for bad in (8, 32, 1 << 9, 1 << 31, 0xFFFFFE08):
            assert trace(LDS | bad) == E.MIRT_ERR_BAD_MODE and radiance(P(4, 0, 8, LDS | bad, 0)) == E.MIRT_ERR_BAD_MODE
        for bad in (2, 3, 16, 64, 1 << 31, 0xFFFFFEFE):
            assert features(params(), LDS | bad) == E.MIRT_ERR_BAD_MODE
        # null pointers
        for a, b in ((None, ph), (pr, None), (None, None)):
            assert trace(LDS, a, b) == E.MIRT_ERR_NULL_POINTER
        for a, b in ((None, qo), (qr, None), (None, None)):
            assert radiance(P(4, 0, 8, LDS, 0), a, b) == E.MIRT_ERR_NULL_POINTER
        assert radiance(None) == E.MIRT_ERR_NULL_POINTER
        assert features(None, LDS) == E.MIRT_ERR_NULL_POINTER and features(params(), LDS, None) == E.MIRT_ERR_NULL_POINTER
        # nothing to do
        assert trace(LDS, None, None, 0) == 0 and radiance(P(4, 0, 8, LDS, 0), None, None, 0) == 0
        assert radiance(P(0, 0, 8, LDS, 0), None, None, 0) == E.MIRT_ERR_SPP_ZERO                 # the checks come before "nothing to do"
        # radiance params
        assert radiance(P(0, 0, 8, LDS, 0)) == E.MIRT_ERR_SPP_ZERO
        assert radiance(P((1 << 24) + 1, 0, 8, LDS, 0)) == E.MIRT_ERR_SPP_RANGE and radiance(P(4, 0xFFFFFFFD, 8, LDS, 0)) == E.MIRT_ERR_SPP_RANGE
        assert radiance(P(4, 0, 8, LDS | m.MIRT_RADIANCE_SKY_HOSEK, 0)) == E.MIRT_ERR_SKY                      # no blob in this scene
        # feature params
        assert features(params(0, 48), LDS) == E.MIRT_ERR_VIEWPORT_SIZE and features(params(64, 0), LDS) == E.MIRT_ERR_VIEWPORT_SIZE
        for rows in (dict(row_begin=30, row_end=20), dict(row_end=49), dict(tile_rows=4, n_parts=3, part=3)):
            assert features(params(**rows), LDS) == E.MIRT_ERR_BAD_ROWS, rows
        assert features(params(spp=_abi.MIRT_MAX_SPP_PER_CALL + 1), LDS) == E.MIRT_ERR_SPP_RANGE
        assert features(params(spp=2, sample_begin=0xFFFFFFFE), LDS) == E.MIRT_ERR_SPP_RANGE
        assert features(params(spp=2, frame_spp=2), LDS) == E.MIRT_ERR_FRAME_SPP and features(params(spp=0, frame_spp=1), LDS) == E.MIRT_ERR_FRAME_SPP
        assert features(params(), LDS, po, pn - 1) == E.MIRT_ERR_OUT_BUFFER and features(params(), LDS, po, 0) == E.MIRT_ERR_OUT_BUFFER
        assert features(params(row_begin=7, row_end=29), LDS, po, 22 * 64 * 32 - 1) == E.MIRT_ERR_OUT_BUFFER
        assert lib.mirt_ctx_trace_stats(ctx._h, None) == E.MIRT_ERR_NULL_POINTER
        assert ctx.last_kernel() == kernel, "a refused call queues nothing"
        for a in (hits, rad_out, feat):
            assert (_bytes(a) == 0xA5).all(), "a refused call writes nothing"
        # the queries leave renders, statistics and sums alone
        p4 = params(spp=4, num_bounces=4)
        ctx.accum_reset(p4)
        ctx.accum_add(p4)
        sums, before = ctx.accum_read(p4), ctx.stats()
        ctx.trace_rays(rays, COUNT, lds=True)
        ctx.render_features(params(spp=1), lds=True)
        ctx.trace_radiance(rad_rays, 2, lds=True)
        assert ctx.last_kernel() == "radiance_rays_lds_kernel<false,true>"
        assert ctx.accum_samples() == 4 and np.array_equal(ctx.accum_read(p4), sums)
        after = ctx.stats()
        assert after["launches"] == 0 and after["kernel_ms_total"] == 0
        assert {k: v for k, v in after.items() if k not in ("launches", "kernel_ms_total")} == {k: v for k, v in before.items() if k not in ("launches", "kernel_ms_total")}
        assert np.array_equal(ctx.render(params(spp=2)), img) and ctx.last_kernel() == kernel
        ctx.set_timing(False)
        ctx.trace_rays(rays, lds=True)
        assert ctx.trace_stats()["kernel_ms"] == 0.0
        ctx.set_timing(True)
        # scenes whose tables a path-traced render refuses: feature frames and radiance answer the same, ray queries read no material
        arr, mats, tex = rr.world()
        broken = arr.copy()
        broken["material_idx"][7] = 99
        ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), broken, mats, tex))
        assert lib.mirt_ctx_render(ctx._h, C.byref(params(spp=1)), po, 64 * 48 * 4) == E.MIRT_ERR_MATERIAL_INDEX
        assert radiance(P(4, 0, 8, LDS, 0)) == E.MIRT_ERR_MATERIAL_INDEX == features(params(), LDS)
        assert len(ctx.trace_rays(rays, lds=True)) == 100
        past = [_abi.MirtMaterial.from_buffer_copy(bytes(x)) for x in mats]
        past[0].desc1.offset = len(np.asarray(tex).reshape(-1, 3))
        ctx.set_scene(hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), arr, past, tex))
        assert features(params(), LDS) == E.MIRT_ERR_TEXEL_RANGE == radiance(P(4, 0, 8, LDS, 0))
        assert (_bytes(rad_out) == 0xA5).all() and (_bytes(feat) == 0xA5).all()


def test_raytracer_queries_leave_the_scene_in_lds():
    scene, cam = m.scenes.three_spheres()
    w, h = 96, 64
    rp = m.RenderParams(camera=cam, viewport_size=(w, h), sampling=m.SamplingParams(max_samples_per_pixel=4, num_samples_per_pixel=4, num_bounces=4))
    rays = m.make_radiance_rays(np.tile([[0.0, 1.0, 4.0]], (64, 1)), np.random.default_rng(2).normal(size=(64, 3)), np.arange(64))
    stay, move = m.Raytracer(scene, rp, device=0), m.Raytracer(scene, rp, device=0)
    try:
        image = stay.render()
        lds_kernel = stay._ctx.last_kernel()
        assert "hbm" not in lds_kernel
        picks = [(x, y) for x in (5, w // 2, w - 7) for y in (3, h // 2, h - 2)]
        a = [stay.pick(x, y, lds=True) for x, y in picks]
        b = [move.pick(x, y) for x, y in picks]
        assert stay._ctx.last_kernel() == "trace_rays_lds_kernel<false,false,false>" and move._ctx.last_kernel() == "trace_rays_kernel<true,false,false>"
        assert any(v is not None for v in a) and any(v is None for v in a)
        for u, v in zip(a, b):
            assert (u is None) == (v is None)
            if u is not None:
                assert u["sphere"] == v["sphere"] and u["t"] == v["t"] and np.array_equal(u["point"], v["point"]) and np.array_equal(u["normal"], v["normal"])
        fa, fb = stay.features(1, lds=True), move.features(1)
        assert stay._ctx.last_kernel() == "feature_frame_lds_kernel<false>"
        for k in ("albedo", "normal", "t", "sphere"):
            assert np.array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32)), k
        assert np.array_equal(stay.radiance(rays, 2, lds=True), move.radiance(rays, 2))
        assert stay._ctx.last_kernel() == "radiance_rays_lds_kernel<false,false>"
        assert not stay._hbm and move._hbm
        assert np.array_equal(stay.render(), image) and stay._ctx.last_kernel() == lds_kernel       # later frames keep their LDS build
        assert np.array_equal(move.render(), image) and "hbm" in move._ctx.last_kernel()
        with pytest.raises(ValueError):
            stay.pick(1, 1, lds=1)
    finally:
        stay.close()
        move.close()
