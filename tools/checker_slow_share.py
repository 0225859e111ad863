#!/usr/bin/env python3
"""How often a wave of the checkerboard routine leaves the fast sign path (csrc/mirt_device_math.h: sin_product_negative).

    make -C weekend-raytracer-wgpu_amd/csrc OUT=../../tools/_scratch/libs/libmirt_diag.so OBJDIR=build/obj_diag EXTRA=-DMIRT_DIAG_CHECKER
    python tools/checker_slow_share.py tools/_scratch/libs/libmirt_diag.so [--scene three_spheres] [--size 1920x1080] [--spp 100]

The diagnosis build counts, per wave that runs the function, whether any of its lanes was undecided (the wave then takes the
branch to the full reduction).  One JSON line per schedule: default, strip, pool.  Needs a GPU."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import weekend_raytracer_wgpu_amd as m  # noqa: E402
from weekend_raytracer_wgpu_amd import _abi  # noqa: E402
from helpers import scene_data  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("lib")
ap.add_argument("--scene", default="three_spheres")
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--spp", type=int, default=100)
a = ap.parse_args()
w, h = map(int, a.size.split("x"))
lib = C.CDLL(str(Path(a.lib).resolve()))
_abi.bind(lib, {k: v for k, v in _abi.SYMBOLS.items() if hasattr(lib, k)})
lib.mirt_diag_checker_sign.restype, lib.mirt_diag_checker_sign.argtypes = C.c_int, [C.POINTER(C.c_uint64), C.c_int]
ctx = C.c_void_p()
assert lib.mirt_ctx_create(0, C.byref(ctx)) == 0
sc = scene_data(a.scene, w, h).as_c()
assert lib.mirt_ctx_set_scene(ctx, C.byref(sc)) == 0
out = np.empty((h, w, 4), np.uint8)
cnt = (C.c_uint64 * 2)()
for name, flags in (("default", 0), ("strip", m.MIRT_FLAG_KERNEL_STRIP), ("pool", m.MIRT_FLAG_KERNEL_POOL)):
    p = m.make_params(w, h, a.spp, mode=m.MIRT_MODE_PT, num_bounces=8, flags=flags)
    assert lib.mirt_diag_checker_sign(cnt, 1) == 0
    assert lib.mirt_ctx_render(ctx, C.byref(p), out.ctypes.data_as(C.c_void_p), out.nbytes) == 0
    assert lib.mirt_diag_checker_sign(cnt, 1) == 0
    print(json.dumps({"scene": a.scene, "size": a.size, "spp": a.spp, "schedule": name, "kernel": lib.mirt_ctx_last_kernel(ctx).decode(),
                      "checker_waves": int(cnt[0]), "slow_waves": int(cnt[1]), "slow_share": cnt[1] / max(1, cnt[0])}))
lib.mirt_ctx_destroy(ctx)
