"""Scenes in which ROUNDING decides a hit, for the LDS grid builds, and a CPU predictor that shows they are not vacuous.

The flat scan (the oracle, the reference's semantics) reports the hits `test_sphere` COMPUTES: with u = 2^-24 and L = |o - c| + |r| a
ray that passes up to about sqrt(35 u) L beside a sphere can have a computed disc > 0.  A grid is exact only if such a "phantom" hit
is found as well.  The scenes below put many of them where a walk through cells binned with the walk's own rounding slack alone
(1e-3 cell, what the builder used before it knew better) cannot find them; `decisive_rays` counts those rays with a plain numpy
restatement of test_sphere and of build_grid (csrc/mirt_api.hip), checked against mirt_grid_plan so that it cannot drift.

Host-side data only; a helper like hbm_worlds.py, not a conftest."""
from __future__ import annotations

import ctypes as C

import numpy as np

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi
from hbm_worlds import SPHERE_DTYPE, field_materials, look, scene_from_arrays, sphere_array

f32 = np.float32
MIN_T, MAX_T = f32(0.001), f32(1000.0)
K_DISC = 35.0 * 2.0 ** -24              # the bound on disc's error, in units of A L^2 (csrc/mirt_kernels.hip, next to kBvhSlack)
GRID_MIN_SPHERES, GRID_MAX_CELLS, GRID_SAFE_REACH = 32, 4096, 2.5


# ------------------------------------------------------------------------------------------ worlds

def sphere_soup(rng, n, spread, r_lo, r_hi, n_big=2):
    """The soup of tests/test_gpu_pt.py::_sphere_soup as arrays: a ground sphere, n_big spheres of radius 1.5, n small ones."""
    cen, rad = [[0.0, -1000.0, 0.0]], [1000.0]
    for _ in range(n_big):
        cen.append(rng.normal(size=3) * spread * 0.3 + (0, 1.5, 0))
        rad.append(1.5)
    for _ in range(n):
        c = rng.normal(size=3) * spread
        c[1] = abs(c[1]) * 0.3 + 0.1
        cen.append(c)
        rad.append(float(rng.uniform(r_lo, r_hi)))
    return np.asarray(cen, np.float64), np.asarray(rad, np.float64)


def _field(seed=1, n_small=480, half=11.0, ground=True):
    """An RTIOW-like field: small spheres of r in [0.15, 0.25] resting on the ground over a square of side 2 x half, three heroes,
    a hollow glass, and (optionally) the 1000-radius ground sphere."""
    rng = np.random.default_rng(seed)
    xz = rng.uniform(-half, half, (n_small, 2))
    r = rng.uniform(0.15, 0.25, n_small)
    cen = np.concatenate([[[0, 1, 0], [0, 1, 0], [-4, 1, 0], [4, 1, 0]], np.stack([xz[:, 0], r, xz[:, 1]], 1)])
    rad = np.concatenate([[1.0, -0.9, 1.0, 1.0], r])
    mat = np.concatenate([[3, 3, 1, 2], rng.integers(0, 7, n_small)])
    if ground:
        cen, rad, mat = np.concatenate([[[0, -1000, 0]], cen]), np.concatenate([[1000.0], rad]), np.concatenate([[4], mat])
    return cen, rad, mat


def adversarial_worlds(lattice_half=6, n_copies=1000):
    """The adversarial worlds of tests/test_gpu_hbm_scene.py (lattice_half = 6) and, cut to LDS size (lattice_half = 5), of the LDS
    grid builds: (name, centres, radii, material indices, eye, at, vfov)."""
    n_mats = len(field_materials()[0])
    out = []
    # copies of one sphere with different materials: the lowest index must win
    k = n_copies
    out.append(("copies", np.tile([[0.0, 0.0, -3.0]], (k, 1)), np.full(k, 0.7), np.arange(k) % n_mats, (0, 0, 1), (0, 0, -3), 60))
    # a tangent lattice: spheres of radius 0.5 on a unit grid, boxes sharing faces, seen along an axis (zero ray components)
    g = np.arange(-lattice_half, lattice_half + 1, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g - 10, indexing="ij")
    lat = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    out.append(("lattice axis", lat, np.full(len(lat), 0.5), np.arange(len(lat)) % n_mats, (0, 0, 8), (0, 0, -10), 40))
    out.append(("lattice oblique", lat, np.full(len(lat), 0.5), np.arange(len(lat)) % n_mats, (9, 7, 5), (0, 0, -10), 40))
    # a camera inside a big sphere, small ones around it
    rng = np.random.default_rng(9)
    cen = np.concatenate([[[0, 0, 0]], rng.uniform(-3, 3, (300, 3))])
    rad = np.concatenate([[5.0], rng.uniform(0.05, 0.3, 300)])
    out.append(("inside", cen, rad, rng.integers(0, n_mats, 301), (0.1, 0.2, 0.3), (1, 0, -2), 70))
    # rays grazing r = 1e-3 spheres at distance ~1e3, zero-radius and non-finite spheres among them
    cen = np.concatenate([rng.uniform(-40, 40, (2000, 2)), np.full((2000, 1), -1000.0)], 1)[:, [0, 1, 2]]
    rad = np.full(2000, 1e-3)
    rad[::7] = 0.0
    cen[5] = [np.inf, 0, -1000]
    cen[11] = [np.nan, 1, -1000]
    rad[17] = np.inf
    rad[23] = np.nan
    out.append(("grazing", cen, rad, rng.integers(0, n_mats, 2000), (0, 0, 0), (0, 0, -1000), 4.5))
    return out


def _scene(cen, rad, mat, cam):
    mats, tex = field_materials()
    return scene_from_arrays(cam, sphere_array(cen, rad, mat), mats, tex)


def grazing(plane="xy"):
    """The finite part of the HBM test's grazing world: r = 1e-3 (every seventh 0) on a plane 1000 away, vfov 4.5.  plane = "xz":
    the plane lies below the eye, the grid is one cell high (the FLATY builds)."""
    _, cen, rad, mat, _, _, vfov = adversarial_worlds()[4]
    keep = np.isfinite(cen).all(1) & np.isfinite(rad)
    cen, rad, mat = cen[keep], rad[keep], mat[keep]
    w, h = 96, 64
    if plane == "xy":
        return _scene(cen, rad, mat, look(w, h, (0, 0, 0), (0, 0, -1000), vfov=vfov)), w, h
    cen = cen[:, [0, 2, 1]]                      # (x, -1000, y): seen from straight above, "up" along -z
    cam = m.Camera(np.zeros(3, f32), np.asarray((0, -1, 0), f32), np.asarray((0, 0, -1), f32), m.Angle.degrees(vfov), 0.0, 10.0)
    return _scene(cen, rad, mat, m.GpuCamera.new(cam, (w, h)).c), w, h


def telephoto(D, ground=True, aperture=0.0):
    """The field seen from D units away, vfov chosen so that the field fills the frame."""
    cen, rad, mat = _field(ground=ground)
    w, h = 96, 64
    eye = np.array([13.0, 2.0, 3.0]) / np.linalg.norm([13.0, 2.0, 3.0]) * D
    vfov = float(np.degrees(2 * np.arctan(10.0 / D)))
    return _scene(cen, rad, mat, look(w, h, eye, (0, 0, 0), vfov=vfov, aperture=aperture, focus=float(D))), w, h


def far_origins():
    """The field in the foreground of a camera low over the 1000-radius ground, looking towards the horizon: many paths reach the
    field by bouncing off ground points hundreds of units away."""
    cen, rad, mat = _field()
    mat = mat.copy()
    mat[0] = 0                                   # a lambertian ground: its bounces go everywhere
    w, h = 96, 64
    return _scene(cen, rad, mat, look(w, h, (16.0, 0.8, 1.0), (-100.0, 0.6, -6.0), vfov=35.0, focus=16.0)), w, h


SOUP = dict(n=400, spread=5.0, r_lo=0.03, r_hi=0.35, at=(0.0, 0.5, 0.0))
SOUP_NEAR = dict(eye=(7.5, 2.5, 6.0), vfov=40.0, focus=9.8)              # next to the soup, as every grid test of test_gpu_pt.py
SOUP_FAR = dict(eye=(1544.0, 308.0, 1234.0), vfov=0.46, focus=2000.0)    # 2000 units away, the soup fills the frame


def _soup(shift=(0.0, 0.0, 0.0), scale=1.0, far=False, seed=31):
    rng = np.random.default_rng(seed)
    cen, rad = sphere_soup(rng, SOUP["n"], SOUP["spread"], SOUP["r_lo"], SOUP["r_hi"])
    mat = rng.integers(0, 7, len(rad))
    shift = np.asarray(shift, np.float64)
    cen, rad = (cen + shift) * scale, rad * scale
    w, h = 96, 64
    cam = SOUP_FAR if far else SOUP_NEAR
    eye, at = (np.asarray(cam["eye"]) + shift) * scale, (np.asarray(SOUP["at"]) + shift) * scale
    return _scene(cen, rad, mat, look(w, h, eye, at, vfov=cam["vfov"], focus=cam["focus"] * scale)), w, h


def soup(far=False):
    """The un-shifted soup: under the near camera the control (the regime of the existing grid tests)."""
    return _soup(far=far)


def translated(k, axes="x", far=False):
    """The soup, camera included, shifted by 2^k along x (or along all three axes): the same geometry at large coordinates.  Under
    the near camera the walk runs at those coordinates; under the far one the sphere tests decide hits as well."""
    s = 2.0 ** k
    return _soup(shift=(s, 0.0, 0.0) if axes == "x" else (s, s, s), far=far)


def scaled(k, far=False):
    """The soup and its camera multiplied by 2^k: the builder's constants must be scale-free."""
    return _soup(scale=2.0 ** k, far=far)


def mixed_radii(seed=5, D=200.0):
    """Radii from 1e-4 to 1 in one scene (median about 1e-2), seen from D units."""
    rng = np.random.default_rng(seed)

    def logu(lo, hi, n):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    rad = np.concatenate([logu(1e-4, 3e-3, 80), logu(3e-3, 3e-2, 480), logu(5e-2, 1.0, 40)])
    n = len(rad)
    cen = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.3, n) + rad, rng.uniform(-1.5, 1.5, n)], 1)
    order = rng.permutation(n)
    w, h = 96, 64
    eye = np.array([40.0, 18.0, 24.0]) / np.linalg.norm([40.0, 18.0, 24.0]) * D
    cam = look(w, h, eye, (0, 0.2, 0), vfov=float(np.degrees(2 * np.arctan(2.2 / D))), focus=float(D))
    return _scene(cen[order], rad[order], rng.integers(0, 7, n), cam), w, h


def degenerate(n_nonfinite):
    """The LDS counterpart of the HBM test's degenerate spheres: zero radii, negative radii (hollow glass), exact duplicates, and
    n_nonfinite spheres with inf / nan centres or radii.  The soup has three big spheres: with 61 non-finite ones the always-tested
    list is full (64), with 65 no grid is built at all."""
    rng = np.random.default_rng(77)
    cen, rad = sphere_soup(rng, 300, 4.0, 0.05, 0.35)
    mat = rng.integers(0, 7, len(rad))
    rad[10:30] = 0.0
    shells = np.arange(40, 60)                                   # hollow glass: an inner sphere of negative radius
    cen, rad, mat = np.concatenate([cen, cen[shells]]), np.concatenate([rad, -0.9 * rad[shells]]), np.concatenate([mat, np.full(20, 3)])
    mat[shells] = 3
    dup = np.arange(70, 80)                                      # exact duplicates, later in the list: the lower index must win
    cen, rad, mat = np.concatenate([cen, cen[dup]]), np.concatenate([rad, rad[dup]]), np.concatenate([mat, (mat[dup] + 1) % 7])
    bad_c, bad_r = rng.uniform(-4, 4, (n_nonfinite, 3)), rng.uniform(0.05, 0.35, n_nonfinite)
    kind = np.arange(n_nonfinite) % 4
    bad_c[kind == 0, 0] = np.inf
    bad_c[kind == 1, 1] = np.nan
    bad_r[kind == 2] = np.inf
    bad_r[kind == 3] = np.nan
    at = rng.integers(3, len(rad), n_nonfinite)                  # scattered through the list
    cen, rad, mat = np.insert(cen, at, bad_c, 0), np.insert(rad, at, bad_r), np.insert(mat, at, rng.integers(0, 7, n_nonfinite))
    w, h = 64, 48
    return _scene(cen, rad, mat, look(w, h, (9.0, 2.0, 7.0), (0, 0.5, 0), vfov=40.0, aperture=0.05, focus=11.0)), w, h


def adversarial_lds(name):
    """`copies`, `lattice axis`, `lattice oblique`, `inside` of the HBM test, cut to LDS size."""
    for nm, cen, rad, mat, eye, at, vfov in adversarial_worlds(lattice_half=5)[:4]:
        if nm == name:
            w, h = 48, 32
            return _scene(cen, rad, mat, look(w, h, eye, at, vfov=vfov)), w, h
    raise KeyError(name)


# name -> (builder, has a grid).  Every scene has 32 .. 2000 spheres and a frame of at most 96 x 64.
SCENES = {
    "grazing xy": (lambda: grazing("xy"), True),
    "grazing xz": (lambda: grazing("xz"), True),
    "telephoto 100": (lambda: telephoto(100.0), True),
    "telephoto 1000": (lambda: telephoto(1000.0), True),
    "telephoto 4000": (lambda: telephoto(4000.0), True),
    "telephoto 1000 lens": (lambda: telephoto(1000.0, aperture=0.05), True),
    "far origins": (far_origins, True),
    "soup": (soup, True),
    "soup far": (lambda: soup(far=True), True),
    "translated 8": (lambda: translated(8), True),
    "translated 12": (lambda: translated(12), True),
    "translated 16": (lambda: translated(16), True),
    "translated 16 xyz": (lambda: translated(16, "xyz"), True),
    "translated 16 far": (lambda: translated(16, far=True), True),
    "translated 16 xyz far": (lambda: translated(16, "xyz", far=True), True),
    "scaled -10": (lambda: scaled(-10), True),
    "scaled +10": (lambda: scaled(10), True),
    "scaled -10 far": (lambda: scaled(-10, far=True), True),
    "scaled +10 far": (lambda: scaled(10, far=True), True),
    "mixed radii": (mixed_radii, True),
    "degenerate 61": (lambda: degenerate(61), True),
    "degenerate 65": (lambda: degenerate(65), False),
    "copies": (lambda: adversarial_lds("copies"), True),
    "lattice axis": (lambda: adversarial_lds("lattice axis"), True),
    "lattice oblique": (lambda: adversarial_lds("lattice oblique"), True),
    "inside": (lambda: adversarial_lds("inside"), True),
}


# ------------------------------------------------------------------------------------------ the predictor

def spheres_of(sd):
    """(centres float32 [n, 3], radii float32 [n]) of a SceneData."""
    n = len(sd.spheres)
    a = np.frombuffer(sd._c_spheres, SPHERE_DTYPE, count=n)
    return a["center"][:, :3].copy(), a["radius"].copy()


def grid_plan(sd, lds=0):
    """mirt_grid_plan of the scene's spheres (host only)."""
    out = _abi.MirtGridPlan()
    c = sd.as_c()
    assert m.lib().mirt_grid_plan(C.cast(c.spheres, C.c_void_p), c.n_spheres, lds, C.byref(out)) == 0, m.lib().mirt_last_error()
    return out


def binning(cen, rad, cell_factor=2.5, big_factor=4.0, disc_slack=True):
    """build_grid's binning (csrc/mirt_api.hip), restated: median radius, big-sphere rule, the enlargement eps, the grid's box grown by
    it, cell growth to kGridMaxCells.  disc_slack=False: the enlargement without its e_disc part -- the walk's own rounding slack
    only, which is what `decisive_rays` holds the scenes against.  None when no grid is built."""
    n = len(rad)
    if n < GRID_MIN_SPHERES or n > 65535:
        return None
    radii = np.abs(rad.astype(f32))
    r_med = np.sort(radii)[n // 2]                      # (NaN sorts last, as nth_element leaves it for these scenes)
    if not (r_med > 0) or not np.isfinite(r_med):
        return None
    finite = np.isfinite(cen).all(1) & np.isfinite(radii)
    with np.errstate(invalid="ignore"):
        big = ~finite | (radii > f32(big_factor) * r_med)
    small = np.nonzero(~big)[0]
    if len(small) < GRID_MIN_SPHERES // 2 or int(big.sum()) > 64:
        return None
    c, r = cen[small].astype(np.float64), radii[small].astype(np.float64)
    lo, hi = (c - r[:, None]).min(0), (c + r[:, None]).max(0)
    r_min, rg = r.min(), float(np.sqrt((0.25 * (hi - lo) ** 2).sum()))
    coord_max = max(np.abs(lo).max(), np.abs(hi).max())
    cell = float(cell_factor) * float(r_med)
    while True:
        l_safe = GRID_SAFE_REACH * rg
        e_disc = np.sqrt(r_min * r_min + K_DISC * l_safe * l_safe) - r_min
        if e_disc > 0.25 * cell:
            e_disc = 0.25 * cell
            l_safe = np.sqrt(((r_min + e_disc) ** 2 - r_min * r_min) / K_DISC)
        dims = None
        for p in range(2):
            steps = float(dims.sum()) if p else 48.0
            e_walk = 1e-3 * cell + 2.0 ** -22 * coord_max + 2.0 ** -23 * (steps + 16.0) * l_safe
            eps = e_walk + e_disc
            glo, ghi = lo - eps, hi + eps
            dims = np.maximum(1.0, np.ceil((ghi - glo) / cell + 1e-6))        # counted in float64: an extent of 2^83 cells is no integer
        if dims.prod() <= GRID_MAX_CELLS:
            dims = dims.astype(np.int64)
            break
        cell *= 1.26
    enl = eps if disc_slack else e_walk
    c0 = np.clip(np.floor((c - r[:, None] - enl - glo) / cell), 0, dims - 1).astype(np.int64)
    c1 = np.clip(np.floor((c + r[:, None] + enl - glo) / cell), 0, dims - 1).astype(np.int64)
    return dict(cell=cell, lo=glo, dims=dims, small=small, c0=c0, c1=c1, n_big=int(big.sum()), l_safe=float(l_safe), eps=float(eps),
                e_disc=float(e_disc), centre=0.5 * (lo + hi), rg=rg, n_entries=int(np.prod(c1 - c0 + 1, axis=1).sum()))


def fma32(a, b, c):
    """fma in fp32: the fp64 product of two floats is exact; the sum is rounded to odd in fp64 and then once to fp32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                        # TwoSum: s + err == p + c exactly
    bits = s.view(np.int64) if s.flags.writeable else s.copy().view(np.int64)
    with np.errstate(invalid="ignore"):
        fix = (err != 0) & np.isfinite(s) & ((bits & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(f32)


def dot32(ax, ay, az, bx, by, bz):
    """dot of csrc / ov_dot of the oracle: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma32(az, bz, fma32(ay, by, ax * bx))


def first_roots(o, d, cen, rad):
    """test_sphere for rays [n, 3] x spheres [k]: the first root above MIN_T each pair computes, +inf where it computes none."""
    with np.errstate(all="ignore"):
        rr = (rad.astype(f32) * rad.astype(f32)).astype(f32)
    return first_roots_rr(o, d, cen, rr)


def first_roots_rr(o, d, cen, rr):
    """first_roots from test records {centre, r * r} (the float32 product PreparedSphere.rr / a BVH record holds)."""
    o, d = o.astype(f32), d.astype(f32)
    a = dot32(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])[:, None]
    inv_a = (f32(1.0) / a).astype(f32)
    with np.errstate(all="ignore"):
        oc = [(o[:, k, None] - cen[None, :, k].astype(f32)).astype(f32) for k in range(3)]
        dd = [np.broadcast_to(d[:, k, None], oc[0].shape) for k in range(3)]
        b = dot32(oc[0], oc[1], oc[2], dd[0], dd[1], dd[2])
        rr = np.asarray(rr, f32)
        cq = (dot32(oc[0], oc[1], oc[2], oc[0], oc[1], oc[2]) - rr[None, :]).astype(f32)
        disc = fma32(b, b, -(a * cq).astype(f32))
        pos = disc > 0
        sq = np.sqrt(np.where(pos, disc, f32(0))).astype(f32)
        t0 = ((-b - sq) * inv_a).astype(f32)
        t1 = ((-b + sq) * inv_a).astype(f32)
        f = np.where(t0 > MIN_T, t0, np.where(t1 > MIN_T, t1, f32(np.inf)))
    return np.where(pos, f, f32(np.inf)).astype(f32)


def flat_scan(o, d, cen, rad, chunk=1024):
    """The flat scan's winner per ray (-1: a miss) and its parameter: min f below MAX_T, ties to the lower index."""
    best = np.full(len(o), -1, np.int64)
    closest = np.full(len(o), MAX_T, f32)
    for i in range(0, len(o), chunk):
        f = first_roots(o[i:i + chunk], d[i:i + chunk], cen, rad)
        j = f.argmin(1)                                          # the first minimum: the lower index
        fj = f[np.arange(len(j)), j]
        hit = fj < MAX_T
        best[i:i + chunk] = np.where(hit, j, -1)
        closest[i:i + chunk] = np.where(hit, fj, MAX_T)
    return best, closest


def camera_rays(cam, w, h, u, v):
    """Pinhole camera rays (cameraMakeRay with a zero lens) through image-plane positions u, v in [0, 1) (v downwards)."""
    eye = np.asarray(cam.eye[:3], f32)
    llc, hor, ver = (np.asarray(x[:3], f32) for x in (cam.lower_left_corner, cam.horizontal, cam.vertical))
    vv = (f32(1.0) - v.astype(f32)).astype(f32)
    d = np.stack([(fma32(vv, np.full_like(vv, ver[k]), fma32(u.astype(f32), np.full_like(vv, hor[k]), llc[k])) - eye[k]).astype(f32)
                  for k in range(3)], 1)
    return np.broadcast_to(eye, d.shape).copy(), d


def lattice_rays(sd, w, h, k):
    """A k x k lattice of directions per pixel from the eye."""
    X, Y, I, J = np.meshgrid(np.arange(w), np.arange(h), np.arange(k), np.arange(k), indexing="ij")
    u = ((X + (I + 0.5) / k) / w).ravel()
    v = ((Y + (J + 0.5) / k) / h).ravel()
    return camera_rays(sd.camera, w, h, u, v)


def decisive_rays(sd, w, h, k=2, cell_factor=2.5, rays=None):
    """How many of the k x k lattice rays per pixel have a flat-scan winner that is a binned sphere NOT listed (under the walk's
    own rounding slack) in any cell the exact ray crosses.  The cells that list a sphere form a box of cells, so "crosses one of
    them" is a slab test of the exact ray (fp64, t >= 0) against that box.  Returns (decisive, phantom winners, hits, rays)."""
    cen, rad = spheres_of(sd)
    g = binning(cen, rad, cell_factor, disc_slack=False)
    if g is None:
        return 0, 0, 0, 0
    o, d = lattice_rays(sd, w, h, k) if rays is None else rays
    best, _ = flat_scan(o, d, cen, rad)
    slot = np.full(len(rad), -1, np.int64)
    slot[g["small"]] = np.arange(len(g["small"]))
    s = np.where(best >= 0, slot[np.maximum(best, 0)], -1)
    sel = np.nonzero(s >= 0)[0]                                   # rays won by a binned sphere
    O, D = o[sel].astype(np.float64), d[sel].astype(np.float64)
    blo = g["lo"] + g["c0"][s[sel]] * g["cell"]
    bhi = g["lo"] + (g["c1"][s[sel]] + 1) * g["cell"]
    with np.errstate(all="ignore"):
        ta, tb = (blo - O) / D, (bhi - O) / D
        par = D == 0
        tn = np.where(par, -np.inf, np.minimum(ta, tb)).max(1)
        tf = np.where(par, np.inf, np.maximum(ta, tb)).min(1)
        outside = (par & ((O < blo) | (O > bhi))).any(1)
    crosses = ~outside & (tn <= tf) & (tf >= 0)
    # a phantom: the exact line passes outside the sphere (fp64 geometry)
    c64, r64 = cen[best[sel]].astype(np.float64), np.abs(rad[best[sel]].astype(np.float64))
    oc = O - c64
    dist2 = (oc * oc).sum(1) - (oc * D).sum(1) ** 2 / (D * D).sum(1)
    phantom = dist2 > r64 * r64
    return int((~crosses).sum()), int(phantom.sum()), int((best >= 0).sum()), len(o)
