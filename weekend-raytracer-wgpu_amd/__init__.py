"""weekend-raytracer-wgpu_amd — MI355X-native per-pixel sphere ray tracer.

Drop-in for ONE hot path of linuxing3/weekend-raytracer-wgpu: `Layer::set_data` and its callees
(reference src/raytracer/layer.rs:264-444), plus the path-traced mode whose behaviours the
reference implements in WGSL (src/raytracer/raytracer.wgsl).  The compute lives in csrc/ (HIP for
gfx950 behind the C ABI of include/mirt.h); this package is the host-side mirror of the
reference's Rust interface.  Import it as `weekend_raytracer_wgpu_amd` (repo-root shim).
"""
from . import _abi
from ._abi import (MIRT_FLAG_COUNT_GRID, MIRT_FLAG_COUNT_WORK, MIRT_FLAG_FAST_MATH, MIRT_FLAG_KERNEL_POOL, MIRT_FLAG_KERNEL_STRIP, MIRT_FLAG_NO_GRID, MIRT_FLAG_NO_SRGB, MIRT_FLAG_NO_TONEMAP, MIRT_FLAG_SKY_HOSEK, MIRT_FLAG_TEXEL_TILES,
                   MIRT_MODE_PARITY, MIRT_MODE_PT, MIRT_FEATURES_FLAT, MIRT_RADIANCE_ACCUMULATE, MIRT_RADIANCE_FLAT, MIRT_RADIANCE_SKY_HOSEK, MIRT_RADIANCE_SORT, MIRT_RADIANCE_POOL, MIRT_ADAPT_FLOOR, MIRT_ADAPT_POOL, MIRT_ADAPT_LDS, MIRT_QUERY_LDS, MIRT_DENOISE_SRC_ACCUM, MIRT_DENOISE_SRC_ADAPT, MIRT_DENOISE_OUT_F32, MIRT_REPROJECT_CLAMP, MIRT_ADAPT_RUN_MAX_STEPS,MIRT_RAYS_SORT, MIRT_RAY_SORT_ORIGIN_BITS, MIRT_RAY_SORT_DIRECTION_BITS, MIRT_NODE_MAX_MEMBERS, MIRT_NODE_RCCL, MIRT_RAY_MISS, MIRT_RAYS_ANY_HIT, MIRT_RAYS_COUNT, MIRT_RAYS_FLAT, MIRT_SCENE_HBM, MIRT_SCENE_BVH_DEVICE, MIRT_BVH_MAX_DEPTH)
from ._lib import LIB_PATH, MirtError, lib
from .context import ADAPT_PIXEL_DTYPE, adapt_active, adapt_run_spp, make_adapt_params, make_adapt_run, make_denoise_params, make_reproject_params, camera_project, BVH_LEAF, BVH_NODE_DTYPE, FEATURE_DTYPE, camera_pixel_ray, RAY_DTYPE, RAY_HIT_DTYPE, RADIANCE_DTYPE, RADIANCE_RAY_DTYPE, SPHERE_DTYPE, Context, make_rays, make_radiance_rays, radiance_mean, ray_sort_codes, SceneData, bvh_plan, bvh_pool_plan, adapt_pool_plan, adapt_lds_plan, adapt_lds_groups, make_params, params_out_row_index, params_out_rows, set_scene_any_size
from .node import Node
from .raytracer import *  # noqa: F401,F403
from . import scenes

__version__ = "0.3.0"
from . import multi_gpu
