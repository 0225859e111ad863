"""MIRT_ADAPT_LDS through the layers that need no device: the flag's value, the two prototypes and the struct across the header, the ctypes
mirror, the package, the crate's source and the C++ mirror; mirt_adapt_lds_plan against a restatement of its formula; mirt_adapt_lds_groups
-- the function every wave of the render stage runs -- against the rule in Python's integers at its corners and on seeded triples; every
error path of both; and the preconditions of the GPU tests' worlds, through mirt_grid_plan."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import adaptive_lds_ref as lr
import adaptive_ref as ar
import hbm_worlds

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mirt.h").read_text()
RS = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
HPP = (ROOT / "weekend-raytracer-wgpu_amd" / "host" / "mirt_host.hpp").read_text()
NEW = {"mirt_adapt_lds_plan": 6, "mirt_adapt_lds_groups": 4}
KEYS = ("threads", "grid", "lds_bytes_per_block", "blocks_per_cu")
MAX_SPP = _abi.MIRT_MAX_SPP_PER_CALL


def test_the_flag_has_one_value_everywhere():
    assert re.search(r"^enum \{ MIRT_ADAPT_LDS = 1u << 3 \};", HEADER, re.M)
    assert len(re.findall(r"\bMIRT_ADAPT_LDS = ", HEADER)) == 1
    assert _abi.MIRT_ADAPT_LDS == 8 == m.MIRT_ADAPT_LDS
    assert re.search(r"pub const MIRT_ADAPT_LDS: u32 = 1 << 3;", RS)
    assert re.search(r"static_assert\(MIRT_ADAPT_LDS == 1u << 3\b", HPP)
    assert _abi.MIRT_ADAPT_POOL == 2                                         # its neighbour did not move; bits 0 and 2 have no name
    assert not re.search(r"MIRT_ADAPT_\w+ = 1u << [02]\b", HEADER)
    assert m.make_adapt_params(4, 32, 4096).flags == 0                       # the default stays
    assert m.make_adapt_params(4, 32, 4096, lds=True).flags == 8 and m.make_adapt_params(4, 32, 4096, True, True).flags == 10
    with pytest.raises(ValueError):
        m.make_adapt_params(4, 32, 4096, lds=1)
    assert m.lib().mirt_version() == (0 << 16) | (4 << 8) | 0                # a new capability, no new version


def test_prototypes_and_struct_across_the_mirrors():
    count = lambda args: len([a for a in args.split(",") if a.strip()])
    lib = m.lib()
    for name, arity in NEW.items():
        h = re.search(r"^int %s\s*\(([^)]*)\)\s*;" % name, HEADER, re.M)
        r = re.search(r"pub fn %s\s*\(([^)]*)\)\s*->\s*c_int;" % name, RS)
        assert h and r, name
        assert count(h.group(1)) == count(r.group(1)) == len(_abi.SYMBOLS[name][1]) == arity, name
        f = getattr(lib, name)                                               # the library exports it
        assert f.restype is C.c_int and list(f.argtypes) == list(_abi.SYMBOLS[name][1])
        call = re.search(r"check\(%s\(([^;]*)\)\);" % name, HPP)             # the C++ mirror calls it with as many arguments
        assert call and count(call.group(1)) == arity, name
    assert re.search(r"^int mirt_adapt_lds_plan\(uint32_t n_spheres, uint32_t n_materials, uint32_t grid_bytes, uint32_t hosek, uint64_t lds_bytes_per_cu, "
                     r"MirtAdaptLdsPlan\* out\);", HEADER, re.M)
    assert re.search(r"^int mirt_adapt_lds_groups\(uint32_t count, uint32_t spp, uint32_t grid_waves, uint32_t\* out_log2\);", HEADER, re.M)
    assert re.search(r"pub fn mirt_adapt_lds_plan\(n_spheres: u32, n_materials: u32, grid_bytes: u32, hosek: u32, lds_bytes_per_cu: u64, out: \*mut MirtAdaptLdsPlan\) -> c_int;", RS)
    assert re.search(r"pub fn mirt_adapt_lds_groups\(count: u32, spp: u32, grid_waves: u32, out_log2: \*mut u32\) -> c_int;", RS)
    P = _abi.MirtAdaptLdsPlan
    assert C.sizeof(P) == 16 and tuple(f[0] for f in P._fields_) == KEYS and all(f[1] is C.c_uint32 for f in P._fields_)
    assert [getattr(P, k).offset for k in KEYS] == [0, 4, 8, 12]
    assert re.search(r"typedef struct MirtAdaptLdsPlan \{ uint32_t threads, grid, lds_bytes_per_block, blocks_per_cu; \} MirtAdaptLdsPlan;", HEADER)
    assert re.search(r"static_assert\(sizeof\(MirtAdaptLdsPlan\) == 16,", HEADER) and re.search(r"_Static_assert\(sizeof\(MirtAdaptLdsPlan\) == 16,", HEADER)
    assert re.search(r"sizeof\(MirtAdaptLdsPlan\) == 16", HPP)
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct MirtAdaptLdsPlan \{(.*?)\n\}", RS, re.S).group(1)
    assert re.findall(r"pub (\w+): u32,", body) == list(KEYS)


# ---- mirt_adapt_lds_plan against the formula ----

@pytest.mark.parametrize("hosek", [False, True], ids=["plain sky", "hosek"])
def test_the_plan_equals_the_formula(hosek):
    sky = 144 if hosek else 0
    flat = [(5, 5), (3, 3), (300, 7), (484, 7), (1, 1), (0, 0), (2000, 40), (3822, 7), (3823, 7), (3000, 600), (4000, 7)]
    for n, mats in flat:
        got = m.adapt_lds_plan(n, mats, 0, hosek)
        assert got == lr.lds_plan(n, mats, 0, hosek), (n, mats, got)
        if got["threads"]:
            assert got == dict(threads=256, grid=0, lds_bytes_per_block=96 + sky + 32 * n + 48 * mats, blocks_per_cu=min(8, 163840 // (96 + sky + 32 * n + 48 * mats)))
    assert m.adapt_lds_plan(3822, 7, 0, hosek)["blocks_per_cu"] == 1 and m.adapt_lds_plan(3823, 7, 0, hosek) == dict.fromkeys(KEYS, 0)      # the budget's border
    # a blob that allows exactly 1, 2 and 8 blocks per CU, and the sizes around them
    for blob, want in ((163840 // 8 - 96 - sky, 8), (163840 // 8 - 96 - sky + 16, 7), (163840 // 2 - 96 - sky, 2), (163840 // 2 - 96 - sky + 16, 1),
                       (120 * 1024 - 240, 1), (16, 8), (25360, 6), (99024, 1)):
        got = m.adapt_lds_plan(4000, 7, blob, hosek)
        assert got == lr.lds_plan(4000, 7, blob, hosek) and got["blocks_per_cu"] == want and got["grid"] == 1, (blob, got)
        assert got["lds_bytes_per_block"] == 96 + sky + blob                                  # the tables do not count beside a blob
    assert m.adapt_lds_plan(4000, 7, 120 * 1024 - 240 + 16, hosek) == dict.fromkeys(KEYS, 0)     # a blob above the budget
    assert m.adapt_lds_plan(4096, 7, 4096, hosek) == dict.fromkeys(KEYS, 0)                   # a grid holds 12-bit sphere ids
    assert m.adapt_lds_plan(4095, 7, 4096, hosek)["blocks_per_cu"] == 8
    # another device: lds_bytes_per_cu = 0 is gfx950's 163 840
    for lds in (65536, 163840, 327680):
        for n, mats, blob in ((484, 7, 0), (484, 7, 28512), (1500, 7, 0)):
            assert m.adapt_lds_plan(n, mats, blob, hosek, lds) == lr.lds_plan(n, mats, blob, hosek, lds), (n, blob, lds)
    assert m.adapt_lds_plan(484, 7, 28512, hosek) == m.adapt_lds_plan(484, 7, 28512, hosek, 163840)
    assert m.adapt_lds_plan(484, 7, 28512, hosek, 4096) == dict.fromkeys(KEYS, 0)             # not one block fits


# ---- mirt_adapt_lds_groups against Python's integers ----

def test_the_groups_rule_at_its_corners():
    for count in (0, 1, 16, 17, 64, 65, 1536, 731, 2 ** 32 - 1):
        for waves in (1, 2, 3, 4, 5, 24, 2 ** 20, 2 ** 32 - 1):
            for spp in (2, 4, 6, 8, 12, 2 ** 24):
                assert m.adapt_lds_groups(count, spp, waves) == lr.lds_groups(count, spp, waves), (count, spp, waves)
    assert [m.adapt_lds_groups(0, 8, w) for w in (1, 2 ** 20)] == [0, 0]                      # an empty list
    assert [m.adapt_lds_groups(1, s, 2 ** 20) for s in (2, 4, 6, 8, 2 ** 24)] == [1, 2, 1, 2, 2]      # the cap: trailing zero bits of spp, at most 2
    assert [m.adapt_lds_groups(c, 8, 1) for c in (1, 16, 17, 64)] == [0, 0, 0, 0]             # one wave always has its unit
    assert [m.adapt_lds_groups(c, 8, 2) for c in (1, 16, 17, 32, 33, 64, 65)] == [2, 2, 2, 2, 1, 1, 0]
    assert [m.adapt_lds_groups(1536, 4, w) for w in (24, 25, 48, 49, 96, 97)] == [0, 1, 1, 2, 2, 2]      # the GPU tests' frame


def test_the_groups_rule_on_seeded_triples():
    rng = np.random.default_rng(20)
    for _ in range(4096):
        count = int(rng.integers(0, 1 << int(rng.integers(1, 33))))
        waves = int(rng.integers(1, 1 << int(rng.integers(1, 25))))
        spp = 2 * int(rng.integers(1, MAX_SPP // 2 + 1)) if rng.integers(0, 2) else 2 << int(rng.integers(0, 24))
        assert m.adapt_lds_groups(count, spp, waves) == lr.lds_groups(count, spp, waves), (count, spp, waves)


def test_every_error_path():
    lib = m.lib()
    plan, out = _abi.MirtAdaptLdsPlan(), C.c_uint32(77)
    assert lib.mirt_adapt_lds_plan(5, 5, 0, 0, 0, None) == _abi.MIRT_ERR_NULL_POINTER
    assert lib.mirt_adapt_lds_plan(5, 5, 0, 0, 0, C.byref(plan)) == _abi.MIRT_OK and plan.threads == 256
    assert lib.mirt_adapt_lds_groups(5, 4, 4, None) == _abi.MIRT_ERR_NULL_POINTER
    for spp in (0, 1, 3, MAX_SPP + 1, MAX_SPP + 2):
        assert lib.mirt_adapt_lds_groups(5, spp, 4, C.byref(out)) == _abi.MIRT_ERR_SPP_RANGE, spp
    assert lib.mirt_adapt_lds_groups(5, 4, 0, C.byref(out)) == _abi.MIRT_ERR_BAD_ROWS
    assert out.value == 77                                                   # a refused call writes nothing
    assert lib.mirt_adapt_lds_groups(5, MAX_SPP, 4, C.byref(out)) == _abi.MIRT_OK and out.value == lr.lds_groups(5, MAX_SPP, 4)
    for bad in ((-1, 4, 4), (5, True, 4), (5, 4, 2 ** 32)):
        with pytest.raises(ValueError):
            m.adapt_lds_groups(*bad)
    with pytest.raises(ValueError):
        m.adapt_lds_plan(-1, 5)
    with pytest.raises(m.MirtError):
        m.adapt_lds_groups(5, 3, 4)


# ---- the GPU tests' worlds ----

def test_the_whole_loop_world_has_a_grid_and_fits_the_flat_layout():
    arr, mats, _ = hbm_worlds.rtiow_field(ar.N_SPHERES)
    gp = lr.grid_plan(arr)
    assert gp["cell_factor"] > 0 and gp["blob_bytes"] % 16 == 0
    assert lr.fits_flat(len(arr), len(mats))
    grid, flat = m.adapt_lds_plan(len(arr), len(mats), gp["blob_bytes"]), m.adapt_lds_plan(len(arr), len(mats))
    assert grid["grid"] == 1 and flat["grid"] == 0 and grid["blocks_per_cu"] >= 5 and flat["blocks_per_cu"] == 8


def test_the_grid_only_world_has_a_grid_and_no_flat_layout():
    assert 3832 <= lr.GRID_ONLY_SPHERES <= 4095
    arr, mats, _ = hbm_worlds.rtiow_field(lr.GRID_ONLY_SPHERES)
    gp = lr.grid_plan(arr)
    assert gp["cell_factor"] > 0
    assert not lr.fits_flat(len(arr), len(mats)) and m.adapt_lds_plan(len(arr), len(mats)) == dict.fromkeys(KEYS, 0)
    plan = m.adapt_lds_plan(len(arr), len(mats), gp["blob_bytes"])
    assert plan["grid"] == 1 and plan["blocks_per_cu"] == 1                  # the largest blob the tests stage: one block per CU


def test_the_five_sphere_scene_has_no_grid():
    import helpers
    sd = helpers.scene_data("main_rs_scene", 16, 8)
    n = len(sd.spheres)
    assert n == 5
    arr = hbm_worlds.sphere_array([list(s.center)[:3] for s in sd.spheres], [s.radius for s in sd.spheres], [s.material_idx for s in sd.spheres])
    assert lr.grid_plan(arr)["cell_factor"] == 0 and m.adapt_lds_plan(n, len(sd.materials))["grid"] == 0
