"""mirt_bvh_pool_plan: the geometry MIRT_FLAG_KERNEL_POOL runs on a MIRT_SCENE_HBM scene, host only (no GPU)."""
import ctypes as C

import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi

LDS_PER_CU = 163840
SLOT_CHOICES = (112, 96, 80, 64)


def _block_bytes(slots, depth, hosek, threads=256):
    """The byte formula of include/mirt.h: camera (+ sky), and per wave a two-queue pool and 64 stacks of `depth` entries."""
    return 96 + (144 if hosek else 0) + threads // 64 * (50 * slots + 384 + 256 * depth)


@pytest.mark.parametrize("hosek", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 14, 21, 32])
def test_plan_obeys_the_byte_formula(depth, hosek):
    p = m.bvh_pool_plan(depth, hosek)
    assert p["threads"] == 256 and p["slots"] in SLOT_CHOICES
    assert p["stack_entries"] == depth
    assert p["lds_bytes_per_block"] == _block_bytes(p["slots"], depth, hosek)
    assert p["waves_per_cu"] % (p["threads"] // 64) == 0 and 4 <= p["waves_per_cu"] <= 16
    blocks = p["waves_per_cu"] // (p["threads"] // 64)
    assert p["lds_bytes_per_block"] * blocks <= LDS_PER_CU
    assert p == m.bvh_pool_plan(depth, hosek, LDS_PER_CU)            # 0 means gfx950's LDS
    # the rule: the largest pools that leave 16 waves; where none does, most waves, the larger pools on a tie
    waves = {s: min(16, LDS_PER_CU // _block_bytes(s, depth, hosek) * 4) for s in SLOT_CHOICES}
    with16 = [s for s in SLOT_CHOICES if waves[s] == 16]
    want = with16[0] if with16 else max(SLOT_CHOICES, key=lambda s: (waves[s], s))
    assert (p["slots"], p["waves_per_cu"]) == (want, waves[want])


def test_known_geometries():
    assert m.bvh_pool_plan(14)["slots"] == 112 and m.bvh_pool_plan(14)["waves_per_cu"] == 16
    assert m.bvh_pool_plan(16)["slots"] == 112 and m.bvh_pool_plan(17)["slots"] == 96        # 112 slots keep 16 waves up to depth 16
    assert m.bvh_pool_plan(21) == dict(threads=256, slots=80, waves_per_cu=16, stack_entries=21, lds_bytes_per_block=_block_bytes(80, 21, False))
    assert m.bvh_pool_plan(32)["waves_per_cu"] == 12 and m.bvh_pool_plan(32)["slots"] == 96


def test_a_tiny_lds_budget_fits_nothing():
    assert m.bvh_pool_plan(21, False, 4096) == dict(threads=0, slots=0, waves_per_cu=0, stack_entries=0, lds_bytes_per_block=0)
    one = _block_bytes(64, 21, False)
    assert m.bvh_pool_plan(21, False, one - 1)["slots"] == 0
    assert m.bvh_pool_plan(21, False, one) == dict(threads=256, slots=64, waves_per_cu=4, stack_entries=21, lds_bytes_per_block=one)


def test_argument_errors():
    lib = m.lib()
    assert lib.mirt_bvh_pool_plan(21, 0, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    out = _abi.MirtBvhPoolPlan(1, 2, 3, 4, 5)
    assert lib.mirt_bvh_pool_plan(_abi.MIRT_BVH_MAX_DEPTH + 1, 0, 0, C.byref(out)) == _abi.MIRT_ERR_BAD_ROWS
    assert out.as_dict() == dict(threads=0, slots=0, waves_per_cu=0, stack_entries=0, lds_bytes_per_block=0)
    assert lib.mirt_bvh_pool_plan(_abi.MIRT_BVH_MAX_DEPTH, 0, 0, C.byref(out)) == 0 and out.stack_entries == _abi.MIRT_BVH_MAX_DEPTH
