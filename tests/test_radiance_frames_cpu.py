"""The frame judge of tests/test_gpu_radiance_frames.py (tests/radiance_frames.py) without a GPU, on the oracle and the helpers alone:
the oracle's sums are additive over sample_begin -- which is what lets a sum of 1-spp frames judge accumulated queries --, the rays
are what they are meant to be, and every fixture is far from trivial, so that records equal to the oracle's say something."""
import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd.context import RADIANCE_DTYPE, RADIANCE_RAY_DTYPE
import feature_ref as fr
import oracle_binding as ob
import radiance_frames as rf
import radiance_ref as rr

BOUNCES = 6                                 # test_gpu_deep_trees.BOUNCES, which the deep frames of the device tests use


def _distinct(sums) -> int:
    return len({tuple(p) for p in np.asarray(sums).reshape(-1, 3).tolist()})


def test_the_oracle_is_additive_over_sample_begin_on_the_fixture():
    sd = fr.fixture_scene()
    one = [rf.frame_sums(sd, fr.W, fr.H, s, 8) for s in range(3)]
    assert one[0].dtype == np.uint64 and one[0].shape == (fr.H, fr.W, 3)
    assert np.array_equal(one[0] + one[1] + one[2], rf.frame_sums(sd, fr.W, fr.H, 0, 8, spp=3))
    assert np.array_equal(one[1] + one[2], rf.frame_sums(sd, fr.W, fr.H, 1, 8, spp=2))
    assert not np.array_equal(one[0], one[1]) and not np.array_equal(one[1], one[2])
    rec = rf.frame_records(sd, fr.W, fr.H, (0, 1, 2), 8)
    assert rec.dtype == RADIANCE_DTYPE and rec.shape == (fr.W * fr.H,) and (rec["samples"] == 3).all() and not rec["_pad"].any()
    assert np.array_equal(rec["sum"], rf.frame_sums(sd, fr.W, fr.H, 0, 8, spp=3).reshape(-1, 3))
    # seed and sample_begin together, as the device test asks them
    both = rf.frame_records(sd, fr.W, fr.H, (5, 6), 8, seed=rr.SEED)
    assert np.array_equal(both["sum"], rf.frame_sums(sd, fr.W, fr.H, 5, 8, seed=rr.SEED, spp=2).reshape(-1, 3))
    assert not np.array_equal(both["sum"], rf.frame_records(sd, fr.W, fr.H, (5, 6), 8)["sum"])


@pytest.mark.parametrize("name,view", rf.DEEP_FRAMES)
def test_the_oracle_is_additive_on_a_deep_world_and_its_frames_are_not_flat(name, view):
    cam = rf.deep_cameras(name)[view]
    sd = rf.deep_scene(name, cam)
    w, h = rf.DEEP_W, rf.DEEP_H
    one = [rf.frame_sums(sd, w, h, s, BOUNCES) for s in range(2)]
    assert np.array_equal(one[0] + one[1], rf.frame_sums(sd, w, h, 0, BOUNCES, spp=2))
    n = [_distinct(s) for s in one]
    print(f"{name} {view}: {n} distinct pixel values of {w * h} at samples 0 and 1")
    assert min(n) >= 1000


def test_the_fixture_frames_are_not_flat():
    for aperture in (0.0, 0.1):
        sums = rf.frame_sums(fr.fixture_scene(aperture), fr.W, fr.H, 0, 8)
        n = _distinct(sums)
        print(f"fixture, aperture {aperture}: {n} distinct pixel values of {fr.W * fr.H}")
        assert n >= 1000 and sums.any(2).mean() > 0.9
    sky = rf.frame_sums(rf.fixture_scene_with_sky(), fr.W, fr.H, 0, 8, hosek=True)
    assert _distinct(sky) >= 1000 and not np.array_equal(sky, rf.frame_sums(fr.fixture_scene(), fr.W, fr.H, 0, 8))
    one, many = (rf.frame_sums(fr.fixture_scene(), fr.W, fr.H, 0, nb) for nb in (1, 300))
    assert _distinct(one) < _distinct(many) and not np.array_equal(many, rf.frame_sums(fr.fixture_scene(), fr.W, fr.H, 0, 8))


def test_frame_rays_are_the_pixels_rays_in_row_major_order():
    pin, lens = fr.fixture_camera(), fr.fixture_camera(aperture=0.1)
    n = fr.W * fr.H
    for cam in (pin, lens):
        rays = rf.frame_rays(cam, fr.W, fr.H, 0)
        assert rays.dtype == RADIANCE_RAY_DTYPE and rays.shape == (n,) and not rays.flags.writeable
        assert np.array_equal(rays["stream"], np.arange(n, dtype=np.uint32)) and not rays["_pad"].any()
        assert rf.frame_rays(cam, fr.W, fr.H, 0) is rays                                    # computed once
        o, d = fr.sample_rays(cam, fr.W, fr.H, [5, 66], [0, 44], 0, 0)                      # pixels (5, 0) and (66, 44)
        for k, i in enumerate((5, 44 * fr.W + 66)):
            assert np.array_equal(rays["origin"][i], o[k]) and np.array_equal(rays["direction"][i], d[k])
    rays = rf.frame_rays(pin, fr.W, fr.H, 0)
    assert fr.is_pinhole(pin) and (rays["origin"] == np.asarray(pin.eye[:3], np.float32)).all()    # a pinhole: every ray starts at the eye
    assert len(np.unique(rays["direction"], axis=0)) == n
    assert not np.array_equal(rays["direction"], rf.frame_rays(pin, fr.W, fr.H, 1)["direction"])    # the jitter follows the sample
    assert not np.array_equal(rays["direction"], rf.frame_rays(pin, fr.W, fr.H, 0, rr.SEED)["direction"])
    lens_rays = rf.frame_rays(lens, fr.W, fr.H, 0)
    assert not fr.is_pinhole(lens) and len(np.unique(lens_rays["origin"], axis=0)) == n          # a lens: an origin per lane


def test_high_streams_come_from_one_row_and_differ_from_streams_0_to_7():
    p = m.make_params(rr.N_STREAMS, rf.TALL, 4, mode=m.MIRT_MODE_PT, row_begin=rf.TALL - 1, row_end=rf.TALL)
    assert ob.out_rows(p) == 1 and ob.out_row_index(p, 0) * rr.N_STREAMS == rf.HIGH_STREAM == 2 ** 32 - 8
    for i in rf.SUBSET[:2]:
        sums = rf.high_stream_sums(i)
        assert sums.shape == (1, rr.N_STREAMS, 3) and sums.nbytes == 192                     # the one row, never the image
    rec = np.concatenate([rf.high_stream_records(i) for i in rf.SUBSET])
    assert rec.dtype == RADIANCE_DTYPE and rec.shape == (8 * rr.N_STREAMS,) and (rec["samples"] == 4).all()
    low = rr.oracle_records(rf.SUBSET)
    differ = (rec["sum"] != low["sum"]).any(1).reshape(len(rf.SUBSET), rr.N_STREAMS).any(1)
    print(f"high streams differ from streams 0..7 on rays {[i for i, x in zip(rf.SUBSET, differ) if x]}")
    assert differ.sum() >= 4 and not differ[rf.SUBSET.index(rr.MISSES_ALL)]                  # the sky alone: no draw decides anything
    rays = rf.high_stream_rays(rf.SUBSET)
    base = rr.rays_and_streams(rf.SUBSET)
    assert rays["stream"].min() == rf.HIGH_STREAM and rays["stream"].max() == 0xFFFFFFFF
    assert np.array_equal(rays["stream"] - np.uint32(rf.HIGH_STREAM), base["stream"])
    assert np.array_equal(rays["origin"], base["origin"]) and np.array_equal(rays["direction"], base["direction"])
    # sample_begin and seed reach the high streams as they reach the low ones
    assert not np.array_equal(rf.high_stream_sums(1, sample_begin=5, seed=rr.SEED), rf.high_stream_sums(1))


def test_the_degenerate_worlds_have_an_oracle():
    for name, arr in rf.degenerate_worlds().items():
        sums = rf.frame_sums(rf.degenerate_scene(arr), rf.SMALL_W, rf.SMALL_H, 0, 8)
        n = _distinct(sums)
        print(f"{name}: {len(arr)} spheres, {n} distinct pixel values of {rf.SMALL_W * rf.SMALL_H}")
        assert sums.any(2).all() and n > 16                                                # light comes back everywhere, and not the same
    empty, one, copies = (rf.frame_sums(rf.degenerate_scene(a), rf.SMALL_W, rf.SMALL_H, 0, 8) for a in rf.degenerate_worlds().values())
    assert not np.array_equal(empty, one) and np.array_equal(one, copies)                  # 1000 copies of a sphere look like the sphere


def test_the_moved_world_differs_from_the_fixture():
    moved = rf.moved_fixture_world()
    arr = fr.fixture().arr
    assert np.array_equal(moved[:5], arr[:5]) and (moved["center"][5:, :3] != arr["center"][5:, :3]).any(1).all()
    assert np.array_equal(moved["material_idx"], arr["material_idx"])
    a, b = (rf.frame_sums(rf.fixture_scene_of(w), fr.W, fr.H, 0, 8) for w in (arr, moved))
    assert (a != b).any(2).mean() > 0.1                                                  # measured: 0.22 of the pixels
