"""The CPU reference of mirt_ctx_trace_rays* and the seeded ray sets its tests use (host-side data only; a helper like
grid_rounding.py, not a conftest).

The reference is the flat scan restated exactly: `grid_rounding.first_roots` is test_sphere's arithmetic (fma32 / dot32), the winner
is the lowest index among the smallest f with f < t_max (strict), point = fma32(t, d, o) per component and normal =
(f32(1) / r) * (point - c) in float32 -- what the path tracer shades with.  A NaN's sign and payload are the one thing IEEE 754 leaves
to the implementation (inf * 0 for a zero-radius winner), so `same_bits` compares bit patterns and lets NaN equal NaN."""
from __future__ import annotations

import functools

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd.context import RAY_DTYPE, RAY_HIT_DTYPE
import hbm_worlds
from grid_rounding import adversarial_worlds, first_roots, fma32

f32 = np.float32
MISS = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------ the reference

def roots_matrix(o, d, cen, rad, chunk=512) -> np.ndarray:
    """f [rays, spheres] float32: the first root above MIN_T each pair computes, +inf where it computes none."""
    return np.concatenate([first_roots(o[i:i + chunk], d[i:i + chunk], cen, rad) for i in range(0, len(o), chunk)]) if len(o) \
        else np.zeros((0, len(rad)), f32)


def resolve(f, o, d, t_max, cen, rad) -> np.ndarray:
    """The hit records (RAY_HIT_DTYPE) of rays (o, d) with per-ray bounds t_max, from their roots matrix f."""
    n = len(o)
    out = np.zeros(n, RAY_HIT_DTYPE)
    out["sphere"] = MISS
    if n == 0 or f.shape[1] == 0:
        return out
    t_max = np.broadcast_to(np.asarray(t_max, f32), (n,))
    j = f.argmin(1)                                            # the first minimum: the lower index
    fj = f[np.arange(n), j]
    with np.errstate(invalid="ignore"):
        hit = fj < t_max                                       # strict; False for a NaN bound
    h = np.nonzero(hit)[0]
    t = fj[h]
    oo, dd = o[h].astype(f32), d[h].astype(f32)
    c, r = cen[j[h]].astype(f32), rad[j[h]].astype(f32)
    with np.errstate(all="ignore"):
        p = np.stack([fma32(t, dd[:, k], oo[:, k].astype(np.float64)) for k in range(3)], 1)
        inv_r = (f32(1.0) / r).astype(f32)
        nrm = (inv_r[:, None] * (p - c).astype(f32)).astype(f32)
    out["sphere"][h] = j[h]
    out["t"][h] = t
    out["point"][h] = p
    out["normal"][h] = nrm
    return out


def trace_ref(o, d, t_max, cen, rad) -> np.ndarray:
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    return resolve(roots_matrix(o, d, cen, rad), o, d, t_max, cen, rad)


def any_hit_of(hits: np.ndarray) -> np.ndarray:
    """What MIRT_RAYS_ANY_HIT writes for rays whose nearest-hit records are `hits`: sphere = 0 or MISS, every other field 0."""
    out = np.zeros(len(hits), RAY_HIT_DTYPE)
    out["sphere"] = np.where(hits["sphere"] == MISS, MISS, 0).astype(np.uint32)
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Per record: every 32-bit word equal, a NaN counting as equal to any NaN."""
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), 8)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 8)
    gf, wf = g.view(f32), w.view(f32)
    nan = np.isnan(gf) & np.isnan(wf)
    nan[:, 1] = False                                          # `sphere` is an integer
    return ((g == w) | nan).all(1)


def rays_of(o, d, t_max=1000.0) -> np.ndarray:
    return m.make_rays(np.asarray(o, f32), np.asarray(d, f32), t_max)


# ------------------------------------------------------------------------------------------ worlds and ray sets

def world_arrays(arr):
    """(centres float32 [n, 3], radii float32 [n]) of a SPHERE_DTYPE array."""
    return arr["center"][:, :3].astype(f32), arr["radius"].astype(f32)


@functools.lru_cache(maxsize=None)
def field_world():
    arr, mats, tex = hbm_worlds.rtiow_field(3000)
    return arr, mats, tex


def adversarial(name):
    """A world of grid_rounding.adversarial_worlds() as a SPHERE_DTYPE array."""
    for nm, cen, rad, mat, *_ in adversarial_worlds():
        if nm == name:
            return hbm_worlds.sphere_array(cen, rad, mat)
    raise KeyError(name)


def scene_of(arr):
    """A SceneData of a SPHERE_DTYPE array with the field's materials (ray queries never read them) and some camera."""
    mats, tex = hbm_worlds.field_materials()
    return hbm_worlds.scene_from_arrays(hbm_worlds.look(64, 48, (0, 2, 9), (0, 0, 0)), arr, mats, tex)


@functools.lru_cache(maxsize=None)
def set_a():
    """field: origins over the rtiow field at heights 0.05 .. 3, directions going down at a shallow angle, lengths 0.25 .. 4."""
    arr, _, _ = field_world()
    rng = np.random.default_rng(77)
    n = 4096
    side = 0.9 * np.sqrt(len(arr) - 5)
    o = np.stack([rng.uniform(-side, side, n), rng.uniform(0.05, 3.0, n), rng.uniform(-side, side, n)], 1)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) * 0.3
    d *= (rng.uniform(0.25, 4.0, n) / np.linalg.norm(d, axis=1))[:, None]
    return arr, o.astype(f32), d.astype(f32)


@functools.lru_cache(maxsize=None)
def set_b():
    """grazing: from the origin towards a random sphere of the grazing world (r = 1e-3 at distance 1000) plus a lateral offset in a
    disc of radius 0.4 -- hundreds of radii beside it, where only rounding can produce a hit."""
    arr = adversarial("grazing")
    cen, _ = world_arrays(arr)
    rng = np.random.default_rng(5)
    n = 4096
    ok = np.nonzero(np.isfinite(cen).all(1))[0]
    pick = ok[rng.integers(0, len(ok), n)]
    rr, phi = 0.4 * rng.uniform(0, 1, n), rng.uniform(0, 2 * np.pi, n)
    d = cen[pick].astype(np.float64) + np.stack([rr * np.cos(phi), rr * np.sin(phi), np.zeros(n)], 1)
    return arr, np.zeros((n, 3), f32), d.astype(f32)


@functools.lru_cache(maxsize=None)
def set_c():
    """lattice: axis-parallel rays (two zero direction components) through the tangent lattice from a half-unit grid of origins, so
    that half of them run exactly between spheres: 27 x 27 origins for each of -z, +x and -y scaled by 2."""
    arr = adversarial("lattice axis")
    g = np.arange(-6.5, 6.51, 0.5)
    gz = g - 10.0
    A, B = (x.ravel() for x in np.meshgrid(g, g, indexing="ij"))
    Ax, Bz = (x.ravel() for x in np.meshgrid(g, gz, indexing="ij"))
    n = len(A)
    o = np.concatenate([np.stack([A, B, np.full(n, 8.0)], 1),                 # along -z
                        np.stack([np.full(n, -8.0), Ax, Bz], 1),              # along +x
                        np.stack([Ax, np.full(n, 8.0), Bz], 1)])              # along -y, twice as fast
    d = np.concatenate([np.tile([[0.0, 0.0, -1.0]], (n, 1)), np.tile([[1.0, 0.0, 0.0]], (n, 1)), np.tile([[0.0, -2.0, 0.0]], (n, 1))])
    return arr, o.astype(f32), d.astype(f32)


SETS = {"A": set_a, "B": set_b, "C": set_c}


@functools.lru_cache(maxsize=None)
def set_roots(name):
    """(f matrix, centres, radii) of a set: computed once, shared by every test that needs a reference for its rays."""
    arr, o, d = SETS[name]()
    cen, rad = world_arrays(arr)
    f = roots_matrix(o, d, cen, rad)
    f.setflags(write=False)
    return f, cen, rad


def set_reference(name, t_max=1000.0) -> np.ndarray:
    arr, o, d = SETS[name]()
    f, cen, rad = set_roots(name)
    return resolve(f, o, d, t_max, cen, rad)


def degenerate_rays(seed=3):
    """Rays no camera produces, aimed into the field: (origins, directions, finite-and-non-zero mask).  Zero directions, one and
    two zero components with either sign of zero, non-finite origin components, directions of length 1e-20 and 1e20."""
    rng = np.random.default_rng(seed)
    base_o = np.stack([rng.uniform(-20, 20, 64), rng.uniform(0.05, 3.0, 64), rng.uniform(-20, 20, 64)], 1).astype(f32)
    base_d = rng.normal(size=(64, 3)).astype(f32)
    base_d[:, 1] = -np.abs(base_d[:, 1])
    O, D = [], []

    def add(o, d):
        O.append(np.asarray(o, f32).reshape(-1, 3))
        D.append(np.broadcast_to(np.asarray(d, f32), O[-1].shape).copy())
    add(base_o, [0.0, 0.0, 0.0])
    add(base_o, [-0.0, 0.0, -0.0])
    for k in range(3):
        for z in (0.0, -0.0):
            d = base_d.copy(); d[:, k] = z                       # one zero component
            add(base_o, d)
            d = np.zeros_like(base_d); d[:] = z; d[:, k] = -1.0 if k == 1 else base_d[:, k]   # two zero components
            add(base_o, d)
    for bad in (np.inf, -np.inf, np.nan):
        for k in range(3):
            o = base_o.copy(); o[::2, k] = bad
            add(o, base_d)
    unit = base_d / np.linalg.norm(base_d, axis=1)[:, None]
    add(base_o, unit * f32(1e-20))
    add(base_o, unit * f32(1e20))
    o, d = np.concatenate(O), np.concatenate(D)
    defined = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    return o, d, defined
