"""What the MIRT_ADAPT_LDS tests share (host-side data only; a helper like adaptive_ref.py, not a conftest; nothing here runs a kernel of
the library): the formula of mirt_adapt_lds_plan and the rule of mirt_adapt_lds_groups restated in Python's integers, mirt_grid_plan of a
sphere array, and the grid-only world -- an rtiow_field too large for the flat layout whose grid blob still fits."""
from __future__ import annotations

import ctypes as C
import functools

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
import adaptive_ref as ar
import hbm_worlds

LDS_PER_CU = 163840                         # gfx950
BUDGET = 120 * 1024                         # mirt_ctx_set_scene's LDS budget for either layout, the sky's 144 bytes counted
CAMERA, SKY = 96, 144
GRID_ONLY_SPHERES = 4000                    # rtiow_field(n), n in 3 832 .. 4 095: a grid, and no flat layout


def lds_plan(n_spheres, n_materials, grid_bytes=0, hosek=False, lds_per_cu=0) -> dict:
    """include/mirt.h, in Python integers."""
    lds_per_cu = lds_per_cu or LDS_PER_CU
    tables = grid_bytes if grid_bytes else 32 * n_spheres + 48 * n_materials
    block = CAMERA + (SKY if hosek else 0) + tables
    if CAMERA + SKY + tables > BUDGET or (grid_bytes and n_spheres > 4095) or block > lds_per_cu:
        return dict(threads=0, grid=0, lds_bytes_per_block=0, blocks_per_cu=0)
    return dict(threads=256, grid=1 if grid_bytes else 0, lds_bytes_per_block=block, blocks_per_cu=min(8, lds_per_cu // block))


def lds_groups(count, spp, grid_waves) -> int:
    """include/mirt.h, in Python integers: log2 of the groups of lanes a pixel's spp samples are dealt to."""
    if count == 0:
        return 0
    g_cap = min(2, (spp & -spp).bit_length() - 1)
    for g in range(g_cap + 1):
        if -(-count // (64 >> g)) >= grid_waves:
            return g
    return g_cap


def grid_plan(arr) -> dict:
    """mirt_grid_plan of a SPHERE_DTYPE array (host only)."""
    out = _abi.MirtGridPlan()
    carr, keep = hbm_worlds.c_spheres(arr)
    assert m.lib().mirt_grid_plan(C.cast(carr, C.c_void_p), len(arr), 0, C.byref(out)) == 0, m.lib().mirt_last_error()
    return {k: getattr(out, k) for k, _ in out._fields_}


def fits_flat(n_spheres, n_materials) -> bool:
    return CAMERA + SKY + 32 * n_spheres + 48 * n_materials <= BUDGET


@functools.lru_cache(maxsize=None)
def _grid_only_field():
    return hbm_worlds.rtiow_field(GRID_ONLY_SPHERES)


def grid_only_scene(w=ar.W, h=ar.H):
    arr, mats, tex = _grid_only_field()
    return hbm_worlds.scene_from_arrays(ar.camera(w, h), arr, mats, tex)
