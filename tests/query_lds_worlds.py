"""Worlds and ray sets of the MIRT_QUERY_LDS tests (tests/test_query_lds_abi.py, tests/test_gpu_query_lds.py): every world fits LDS in at
least one layout, so that one context can hold it there and a second one as a MIRT_SCENE_HBM scene.  Everything here is host arithmetic."""
import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
import feature_ref as fr
import grid_rounding as gr
import hbm_worlds
import radiance_ref as rad
import ray_query_ref as rq

f32 = np.float32
T_MAXES = (1000.0, 0.5, 1e-3, 0.0, -1.0, 1e30, np.inf, np.nan)
ADVERSARIAL = ("copies", "lattice axis", "lattice oblique", "inside")


def _arr_scene(arr, w=64, h=48, sky=None):
    mats, tex = hbm_worlds.field_materials()
    return hbm_worlds.scene_from_arrays(hbm_worlds.look(w, h, (13, 2, 3), (0, 0.5, 0), vfov=25), arr, mats, tex, sky)


def main_rs():
    """The five spheres of main.rs: no grid (fewer than 32 spheres), the flat tables."""
    scene, cam = m.scenes.main_rs_scene()
    return m.SceneData(m.GpuCamera.new(cam, (64, 48)).c, [s.to_c() for s in scene.spheres], *m.flatten_materials(scene.materials))


# name -> (builder of the SceneData, has a grid, has the flat tables)
WORLDS = {
    "fixture": (lambda: fr.fixture_scene(), True, True),                          # rtiow_field(3000): an 84 KB blob, 96 KB of flat tables
    "main.rs": (main_rs, False, True),
    "field 484": (lambda: _arr_scene(hbm_worlds.rtiow_field(484)[0]), True, True),
    "grazing": (lambda: rq.scene_of(rq.set_b()[0]), True, True),                  # ray set B's world
    "lattice": (lambda: rq.scene_of(rq.set_c()[0]), True, True),                  # ray set C's world
    "far origins": (lambda: gr.far_origins()[0], True, True),
    "field 4000": (lambda: _arr_scene(hbm_worlds.rtiow_field(4000)[0]), True, False),   # grid only: a 99 KB blob, one block per CU
    "radiance": (lambda: _arr_scene(rad.world()[0]), True, True),                 # rtiow_field(300), the world of radiance_ref's ray set
    "radiance sky": (lambda: _arr_scene(rad.world()[0], sky=rad.sky_blob()), True, True),
}
for _name in ADVERSARIAL:
    WORLDS[_name] = (functools.partial(lambda n: gr.adversarial_lds(n)[0], _name), True, True)


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name][0]()


@functools.lru_cache(maxsize=None)
def spheres(name):
    """(centres float32 [n, 3], radii float32 [n]) of a world."""
    return gr.spheres_of(world(name))


def _eye(name):
    return np.asarray(world(name).camera.eye[:3], np.float64)


def _finite(name):
    cen, rad = spheres(name)
    return np.nonzero(np.isfinite(cen).all(1) & np.isfinite(rad) & (np.abs(rad) < 100.0))[0]


@functools.lru_cache(maxsize=None)
def aimed_rays(name, n=512, seed=41):
    """Rays from around the world's camera towards random small spheres with a lateral jitter of a few radii, lengths 0.25 .. 4; every
    eighth from 300 .. 3000 units away (a far origin where the grid has a guard)."""
    cen, rad = spheres(name)
    rng = np.random.default_rng(seed)
    ok = _finite(name)
    pick = ok[rng.integers(0, len(ok), n)]
    o = _eye(name) + rng.uniform(-0.5, 0.5, (n, 3))
    far = np.arange(n) % 8 == 7
    out = rng.normal(size=(n, 3))
    out[:, 1] = np.abs(out[:, 1])
    o[far] = cen[pick[far]] + out[far] / np.linalg.norm(out[far], axis=1)[:, None] * rng.uniform(300.0, 3000.0, (int(far.sum()), 1))
    at = cen[pick].astype(np.float64) + rng.normal(size=(n, 3)) * (1.5 * np.abs(rad[pick]).astype(np.float64) + 1e-3)[:, None]
    d = at - o
    d *= (rng.uniform(0.25, 4.0, n) / np.linalg.norm(d, axis=1))[:, None]
    return o.astype(f32), d.astype(f32)


@functools.lru_cache(maxsize=None)
def long_t_rays(name, n=256, seed=43):
    """Directions of length 1e-3 towards spheres a few units away: the hits lie at t in the thousands, beyond the renderer's MAX_T."""
    cen, rad = spheres(name)
    rng = np.random.default_rng(seed)
    ok = _finite(name)
    near = ok[np.argsort(np.linalg.norm(cen[ok] - _eye(name), axis=1))[:max(8, len(ok) // 4)]]
    pick = near[rng.integers(0, len(near), n)]
    o = _eye(name) + rng.uniform(-0.25, 0.25, (n, 3))
    at = cen[pick].astype(np.float64) + rng.normal(size=(n, 3)) * (0.5 * np.abs(rad[pick]).astype(np.float64))[:, None]
    d = at - o
    d *= (1e-3 / np.linalg.norm(d, axis=1))[:, None]
    return o.astype(f32), d.astype(f32)


def ray_sets(name):
    """name -> (origins, directions, mask of the rays the CPU reference is defined for) of a world's ray sets."""
    sets = {}
    for key, (o, d) in (("aimed", aimed_rays(name)), ("long t", long_t_rays(name))):
        sets[key] = (o, d, np.ones(len(o), bool))
    if name == "fixture":
        _, o, d = rq.set_a()
        sets["A"] = (o, d, np.ones(len(o), bool))
        sets["degenerate"] = rq.degenerate_rays()
    if name == "grazing":
        _, o, d = rq.set_b()
        sets["B"] = (o, d, np.ones(len(o), bool))
    if name == "lattice":
        _, o, d = rq.set_c()
        sets["C"] = (o, d, np.ones(len(o), bool))
    if name == "field 484":
        sets["degenerate"] = rq.degenerate_rays()
    return sets


@functools.lru_cache(maxsize=None)
def roots(name, key):
    """The roots matrix of a world's ray set (the defined rays only): computed once."""
    o, d, ok = ray_sets(name)[key]
    cen, rad = spheres(name)
    f = rq.roots_matrix(o[ok], d[ok], cen, rad)
    f.setflags(write=False)
    return f


def reference(name, key, t_max):
    """RAY_HIT_DTYPE records of the defined rays of a set under one t_max for all."""
    if key in ("A", "B", "C"):
        return rq.set_reference(key, t_max)          # ray_query_ref's own cache, shared with tests/test_gpu_trace_rays.py
    o, d, ok = ray_sets(name)[key]
    cen, rad = spheres(name)
    return rq.resolve(roots(name, key), o[ok], d[ok], np.full(int(ok.sum()), t_max, f32), cen, rad)
