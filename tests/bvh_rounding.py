"""Ray sets and worlds on which the SLACK of the HBM BVH walk (nearest_hit_bvh: the lateral growth E of every box and kBvhSlack)
decides records, with their references and the mutant walks that show it (host-side data only; a helper like ray_query_ref.py,
not a conftest).

The flat scan reports the hits test_sphere COMPUTES; a "phantom" is a winner whose exact line (fp64 geometry) passes outside its
sphere, by a "reach" of (lateral distance - |r|) / L with L = |o - c| + |r|.  DESIGN.md 10.1 bounds the reach by sqrt(35 u) =
2^-9.4; the walk grows its boxes by 2^-8 L.  A walk that grew them by less would lose phantoms -- on these sets, and on nothing the
suite had before them.  Every set has at most 4096 rays, every world at most 2000 spheres (it fits the LDS builds and the oracle
too); every ray is bounded by t_max = +inf.

  far         a 16 x 16 jittered plane lattice seen from 1e3 .. 1e19 away, radii 0.2 and 1e-3
  translated  the lattice (r = 1e-3) and rays from 1e3 away, shifted by 2^12, 2^16, 2^20 along x / along all three axes
  searched    the worst phantoms a directed search finds (see `searched`), against spheres strung along a line, whose boxes are thin
  near big    origins on or just off spheres of r = 1 grazing them, small spheres (r = 1e-2) just ahead: closest |d| << r_max
  poles       six spheres of r = 1 with a pole at the origin, spheres of r = 2e-5 a hair ahead: the search for the 2 r_max term, kept
  range ends  aimed rays into a field with |d| = 2^-60 .. 2^-66 and 2^55 .. 2^63: where 1 / a overflows and b * b does
"""
from __future__ import annotations

import functools

import numpy as np

from bvh_check import always_list, assemble, check_bvh
from bvh_walk_ref import E_SCALE, SLACK, walk
from grid_rounding import _field, first_roots
from hbm_worlds import sphere_array
import ray_query_ref as rq

f32 = np.float32
T_MAX = f32(np.inf)
REACH_BOUND = 2.0 ** -9.4                   # sqrt(35 u), u = 2^-24 (csrc/mirt_kernels.hip, above kBvhSlack)
FLOOR = 16                                  # records a mutant must change to count as a witness (as tests/test_gpu_deep_trees.py)
FAR_DISTANCES = {"1e3": 1e3, "1e5": 1e5, "1e7": 1e7, "1e10": 1e10, "1e15": 1e15, "1e19": 1e19}
RADII = {"0.2": 0.2, "1e-3": 1e-3}
SHIFTS = (12, 16, 20)
N_RAYS = 4096


# ------------------------------------------------------------------------------------------ worlds and rays

def lattice(r: float, seed: int = 41):
    """(centres float64 [256, 3], radii [256]): a 16 x 16 unit lattice in the plane z = 0, every centre jittered by +-0.25 in the
    plane and +-0.05 off it.  Equal radii: nothing goes to the always-tested list."""
    rng = np.random.default_rng(seed)
    g = np.arange(16, dtype=np.float64) - 7.5
    X, Y = np.meshgrid(g, g, indexing="ij")
    cen = np.stack([X.ravel(), Y.ravel(), np.zeros(256)], 1)
    cen += rng.uniform(-1, 1, (256, 3)) * (0.25, 0.25, 0.05)
    return cen, np.full(256, float(r))


def aimed_from(cen, rad, dist, spread, seed, n=N_RAYS):
    """Origins in the column over the lattice, `dist` above its plane (x, y uniform over the lattice's +-8), each ray aimed at a
    point within `spread` of a random sphere's centre; directions 0.25 .. 4 long.  float64.  Seen from there the rays are nearly
    parallel to z but never exactly: their x and y slabs resolve a lateral miss sharply, and a relative slack on the parameter
    (kBvhSlack) does not hide what E is there for."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), np.full(n, float(dist))], 1)
    v = rng.normal(size=(n, 3))
    v *= (spread * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    at = cen[rng.integers(0, len(cen), n)] + v
    d = at - o
    d *= (rng.uniform(0.25, 4.0, n) / np.linalg.norm(d, axis=1))[:, None]
    return o, d


def _as_set(cen, rad, o, d, mats=None):
    arr = sphere_array(cen, rad, np.arange(len(rad)) % 7 if mats is None else mats)
    o, d = np.asarray(o).astype(f32), np.asarray(d).astype(f32)
    for a in (o, d):
        a.setflags(write=False)
    return arr, o, d


def far(dist_name: str, r_name: str):
    cen, rad = lattice(RADII[r_name])
    o, d = aimed_from(cen, rad, FAR_DISTANCES[dist_name], 3.0 * RADII[r_name], seed=100 + list(FAR_DISTANCES).index(dist_name))
    return _as_set(cen, rad, o, d)


def translated(k: int, axes: str):
    """The r = 1e-3 lattice and rays from 1e3 above it, shifted by 2^k in float64 and then rounded to float32: at 2^20 a coordinate
    resolves 2^-3, 125 radii -- and the 2^-20 (|c| + |r|) pad of a sphere's box is a whole unit along a shifted axis.  The aim
    spread is 0.1: from 1e3 away a phantom reaches up to 2^-11 x 1e3 = 0.5 beside its sphere, so an aim 0.1 off is well inside
    what the flat scan reports and 100 radii outside the sphere's box."""
    cen, rad = lattice(1e-3)
    o, d = aimed_from(cen, rad, 1e3, 0.1, seed=200 + k)
    shift = np.array([2.0 ** k, 0.0, 0.0]) if axes == "x" else np.full(3, 2.0 ** k)
    return _as_set(cen + shift, rad, o + shift, d)


# -- searched

LINE_N, LINE_STEP = 64, 6.0
LINE_RADII = (1.0e-3, 2.0e-3, 3.5e-3)       # within 4 median radii of each other: all of them stay in the tree
# (distance, unit direction of travel): two zero components, one, none
SEARCH_FAMILIES = [(dist, np.asarray(u, np.float64) / np.linalg.norm(u))
                   for dist in (1.0e2, 1.0e3, 1.0e4)
                   for u in ((0.0, 0.0, -1.0), (0.0, -1.0, 0.0), (0.6, 0.0, -0.8), (0.3, -0.5, -0.8), (0.02, 0.01, -1.0), (0.3, -0.02, -0.8),
                             (-0.01, 1.0, 0.03))]
SEARCH_TARGETS, SEARCH_STEPS, SEARCH_KEEP = 8, 384, 96


def line_world():
    """64 spheres strung along the x axis, 6 apart (jittered along x only), radii 1e-3 .. 3.5e-3: every box of every tree over them
    is a piece of the tube |y|, |z| <= 3.5e-3 (plus its 2^-20 pad), so a line that stays farther than that from the axis meets no
    box at all, whatever the builder made of the leaves."""
    rng = np.random.default_rng(43)
    x = (np.arange(LINE_N) - LINE_N / 2) * LINE_STEP + rng.uniform(-1, 1, LINE_N)
    cen = np.stack([x, np.zeros(LINE_N), np.zeros(LINE_N)], 1)
    rad = np.asarray(LINE_RADII)[np.arange(LINE_N) % 3]
    return cen, rad


def reach_of(o, d, cen, rad, winner):
    """(lateral distance of the exact line of ray (o, d) from its winner's centre - |r|) / (|o - c| + |r|) in float64, for float32
    inputs as the device holds them; -inf for a miss.  Positive: a phantom."""
    o, d = np.asarray(o, f32).astype(np.float64), np.asarray(d, f32).astype(np.float64)
    hit = winner >= 0
    j = np.where(hit, winner, 0)
    c, r = cen.astype(f32).astype(np.float64)[j], np.abs(rad.astype(f32).astype(np.float64))[j]
    oc = o - c
    with np.errstate(all="ignore"):
        dn = d / np.sqrt((d * d).sum(1))[:, None]
        perp = oc - (oc * dn).sum(1)[:, None] * dn
        reach = (np.sqrt((perp * perp).sum(1)) - r) / (np.sqrt((oc * oc).sum(1)) + r)
    return np.where(hit, reach, -np.inf)


def winners(f, t_max=T_MAX):
    """The flat scan's winner per ray of a roots matrix (-1: a miss)."""
    if f.shape[1] == 0:
        return np.full(len(f), -1, np.int64)
    j = f.argmin(1)
    return np.where(f[np.arange(len(f)), j] < t_max, j, -1)


@functools.lru_cache(maxsize=None)
def searched():
    """A directed search for the worst phantoms of the flat scan, against first_roots alone (no tree): for every family (distance,
    direction of travel u) and 8 target spheres of the line world a ray runs along u past the target at a lateral offset of
    |r| + x L along w = u x e_x (perpendicular to the ray AND to the line: the offset is the ray's distance from the x axis), x
    swept over 2^-14 .. 2^-9 in 384 steps on both sides (the distance varies by a few percent from target to target).  Of each family the 96 rays whose winner is a phantom with the largest
    reach are kept, and the 96 with the smallest positive reach: 21 families x 192 = 4032 rays at most.
    Families: travel along an axis (two zero components), in a coordinate plane (one), oblique, and nearly along an axis with small
    non-zero components -- the last kind is where a slab resolves a lateral miss sharply."""
    cen, rad = line_world()
    ex = np.array([1.0, 0.0, 0.0])
    targets = np.arange(SEARCH_TARGETS) * (LINE_N // SEARCH_TARGETS) + 3
    xs = np.concatenate([2.0 ** np.linspace(-14.0, -9.0, SEARCH_STEPS // 2), -(2.0 ** np.linspace(-14.0, -9.0, SEARCH_STEPS // 2))])
    O, D = [], []
    for fam, (dist, u) in enumerate(SEARCH_FAMILIES):
        w = np.cross(u, ex)
        w /= np.linalg.norm(w)
        T, X = (a.ravel() for a in np.meshgrid(targets, xs, indexing="ij"))
        far_ = dist * (1.0 + 0.0137 * (T % 7))                                          # no round numbers: their squares would be exact
        L = far_ + rad[T]
        off = np.sign(X) * (rad[T] + np.abs(X) * L)
        o = (cen[T] - far_[:, None] * u + off[:, None] * w).astype(f32)
        d = np.broadcast_to((u * (0.4391 + 0.2713 * (fam % 4))).astype(f32), o.shape)   # lengths 0.44 .. 1.25
        f = np.concatenate([first_roots(o[i:i + 1024], d[i:i + 1024], cen, rad) for i in range(0, len(o), 1024)])
        reach = reach_of(o, d, cen, rad, winners(f))
        order = np.argsort(-reach, kind="stable")
        order = order[reach[order] > 0]
        keep = np.unique(np.concatenate([order[:SEARCH_KEEP], order[::-1][:SEARCH_KEEP]]))
        O.append(o[keep])
        D.append(d[keep])
    return _as_set(cen, rad, np.concatenate(O), np.concatenate(D))


# -- near a big sphere

def near_big(seed: int = 47):
    """320 spheres of r = 1 on a jittered 3-apart lattice (8 x 8 x 5) and 256 of r = 1e-2, each at a "site": a point 0.02 .. 0.2 along
    a tangent of a big sphere, 5e-3 below to 1e-2 above the tangent plane.  The median radius is 1, so the big ones stay in the
    tree and r_max = 1.  Every site gets 16 rays that start on or up to 2e-3 off the big sphere (a few below its surface), up to
    0.05 behind the tangent point, and aim within 1.5 small radii beside and one above or below the small sphere's centre, so that
    they pass the tangent point at a slope of a few hundredths, many within 1e-3 of the big sphere's surface: once the small
    sphere is hit, closest |d| is a hundredth of r_max, while the big sphere the ray grazes -- whose computed root may lie on
    either side of that hit -- has L >= 1.  Half of the sites sit at a pole of their sphere (normal +-x, +-y, +-z), where the
    grazing ray runs OUTSIDE the big sphere's box and only the growth of that box brings the walk to it."""
    rng = np.random.default_rng(seed)
    G = np.stack([a.ravel() for a in np.meshgrid(np.arange(8.0), np.arange(8.0), np.arange(5.0), indexing="ij")], 1)
    big = (G - G.mean(0)) * 3.0 + rng.uniform(-0.3, 0.3, G.shape)
    sites, per = 256, N_RAYS // 256
    host = rng.integers(0, len(big), sites)
    nrm = rng.normal(size=(sites, 3))
    pole = np.zeros((sites // 2, 3))
    pole[np.arange(sites // 2), rng.integers(0, 3, sites // 2)] = rng.choice([-1.0, 1.0], sites // 2)
    nrm[::2] = pole
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    tan = np.cross(nrm, rng.normal(size=(sites, 3)))
    tan /= np.linalg.norm(tan, axis=1)[:, None]
    top = big[host] + nrm                                            # the tangent points
    small = top + rng.uniform(0.02, 0.2, sites)[:, None] * tan + rng.uniform(-5.0e-3, 1.0e-2, sites)[:, None] * nrm
    S = np.repeat(np.arange(sites), per)
    n = len(S)
    off = rng.choice([0.0, 1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 2e-3, -1e-6, -1e-4], n)
    o = top[S] + off[:, None] * nrm[S] - rng.uniform(0.0, 0.05, n)[:, None] * tan[S]
    v = rng.uniform(-1.5e-2, 1.5e-2, n)[:, None] * np.cross(tan[S], nrm[S]) + rng.uniform(-1.0e-2, 1.0e-2, n)[:, None] * nrm[S]
    d = small[S] + v - o
    d *= (rng.uniform(0.25, 4.0, n) / np.linalg.norm(d, axis=1))[:, None]
    cen = np.concatenate([big, small])
    rad = np.concatenate([np.ones(len(big)), np.full(sites, 1e-2)])
    order = rng.permutation(len(rad))                               # big and small mixed through the list
    return _as_set(cen[order], rad[order], o, d)


def poles(seed: int = 71):
    """The directed search for a ray that needs the 2 r_max term, kept as a set.  Six spheres of r = 1 centred at +-e_k share a pole
    at the world's origin, where float32 resolves 1e-11; 48 more of r = 1 stand 20 away (the median radius stays 1); 40 spheres of
    r = 2e-5 lie 5e-5 .. 3e-4 from the origin, each next to the tangent plane of one of the six.  A ray starts 0 .. 3e-6 above that
    plane within 3e-5 of the pole and aims at a point 0 .. 3e-6 above it within 1.5e-5 of its small sphere's foot, |d| = 1e-3 .. 1:
    it grazes a sphere with L = 2 and finds a hit whose closest |d| is 1e-4 of r_max."""
    rng = np.random.default_rng(seed)
    six = np.concatenate([np.eye(3), -np.eye(3)])
    G = np.stack([a.ravel() for a in np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(3.0), indexing="ij")], 1)
    away = (G - G.mean(0)) * 3.0 + (20.0, 0.0, 0.0)
    n_small, n = 40, N_RAYS
    sh = np.arange(n_small) % 6
    sn = -six[sh]                                                   # the outward normal of the host at the origin
    u = np.cross(sn, rng.normal(size=(n_small, 3)))
    u /= np.linalg.norm(u, axis=1)[:, None]
    small = u * rng.uniform(5e-5, 3e-4, n_small)[:, None] + sn * rng.uniform(-1e-5, 1e-5, n_small)[:, None]
    cen = np.concatenate([six, away, small])
    rad = np.concatenate([np.ones(6 + len(away)), np.full(n_small, 2e-5)])
    S = rng.integers(0, n_small, n)
    nrm = sn[S]
    heights = np.array([0.0, 1e-7, 3e-7, 1e-6, 3e-6])
    t1 = np.cross(nrm, rng.normal(size=(n, 3)))
    t1 /= np.linalg.norm(t1, axis=1)[:, None]
    o = nrm * rng.choice(heights, n)[:, None] + t1 * rng.uniform(0, 3e-5, n)[:, None]
    foot = small[S] - nrm * (small[S] * nrm).sum(1)[:, None]
    t2 = np.cross(nrm, rng.normal(size=(n, 3)))
    t2 /= np.linalg.norm(t2, axis=1)[:, None]
    d = foot + t2 * rng.uniform(0, 1.5e-5, n)[:, None] + nrm * rng.choice(heights, n)[:, None] - o
    d *= (10.0 ** rng.uniform(-3, 0, n) / np.linalg.norm(d, axis=1))[:, None]
    return _as_set(cen, rad, o, d)


# -- range ends

RANGE_EXPONENTS = tuple(range(-66, -59)) + tuple(range(55, 64))      # 16 lengths x 256 rays


def range_ends(seed: int = 53):
    """Rays aimed into grid_rounding's field (485 spheres, the ground of radius 1000 on the always-tested list) from 5 .. 25 away,
    within 1.5 radii of a random sphere, 256 for each direction length 2^-66 .. 2^-60 and 2^55 .. 2^63.  At 2^-65 and below
    1 / a overflows (a = |d|^2 is subnormal or zero) and nothing hits, at 2^-64 37 of the 256 rays still do; at the long lengths every root
    distance / |d| lies below MIN_T, and from about 2^60 on b * b overflows and disc is inf - inf: nothing hits either (at 2^64 a
    itself would overflow).  The answer may be "no hit": tree
    and flat scan must agree on it."""
    cen, rad, mat = _field()
    rng = np.random.default_rng(seed)
    per = N_RAYS // len(RANGE_EXPONENTS)
    O, D = [], []
    for e in RANGE_EXPONENTS:
        pick = rng.integers(5, len(rad), per)
        o = np.stack([rng.uniform(-15, 15, per), rng.uniform(0.3, 6.0, per), rng.uniform(-15, 15, per)], 1)
        at = cen[pick] + rng.uniform(-1.5, 1.5, (per, 3)) * np.abs(rad[pick])[:, None] / np.sqrt(3.0)
        d = at - o
        d *= (2.0 ** e / np.linalg.norm(d, axis=1))[:, None]
        O.append(o)
        D.append(d)
    return _as_set(cen, rad, np.concatenate(O), np.concatenate(D), mat)


# ------------------------------------------------------------------------------------------ the sets by name

SETS = {}
for _d in FAR_DISTANCES:
    for _r in RADII:
        SETS[f"far {_d} r={_r}"] = functools.partial(far, _d, _r)
for _k in SHIFTS:
    for _ax in ("x", "xyz"):
        SETS[f"translated 2^{_k} {_ax}"] = functools.partial(translated, _k, _ax)
SETS["searched"] = searched
SETS["near big"] = near_big
SETS["poles"] = poles
SETS["range ends"] = range_ends

FAR = [n for n in SETS if n.startswith("far ")]
TRANSLATED_X = [n for n in SETS if n.startswith("translated") and n.endswith(" x")]
NEED_SLACK = FAR + TRANSLATED_X + ["searched"]       # the sets on which a walk without E must change >= FLOOR records
AUDITED = FAR + ["searched"]                         # the sets whose device trees are audited with the numpy walk


@functools.lru_cache(maxsize=None)
def ray_set(name: str):
    """(world SPHERE_DTYPE, origins, directions float32 [n, 3]); the rays read-only, shared."""
    arr, o, d = SETS[name]()
    assert len(o) <= N_RAYS and 32 <= len(arr) <= 2000
    return arr, o, d


@functools.lru_cache(maxsize=None)
def set_roots(name: str):
    """(f matrix, centres, radii) of a set: computed once, shared by every test that needs a reference for its rays."""
    arr, o, d = ray_set(name)
    cen, rad = rq.world_arrays(arr)
    f = rq.roots_matrix(o, d, cen, rad)
    f.setflags(write=False)
    return f, cen, rad


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    """The flat scan's records (ray_query_ref.resolve) under t_max = +inf; read-only."""
    _, o, d = ray_set(name)
    f, cen, rad = set_roots(name)
    ref = rq.resolve(f, o, d, T_MAX, cen, rad)
    ref.setflags(write=False)
    return ref


def rays_of(name: str) -> np.ndarray:
    _, o, d = ray_set(name)
    return rq.rays_of(o, d, T_MAX)


def reaches(name: str) -> np.ndarray:
    """reach_of every ray's flat-scan winner."""
    _, o, d = ray_set(name)
    f, cen, rad = set_roots(name)
    return reach_of(o, d, cen, rad, winners(f))


@functools.lru_cache(maxsize=None)
def audit_subset(name: str) -> np.ndarray:
    """The fixed rays (at most 1024) on which a tree read back from the device is audited: those whose flat-scan winner has the
    largest reach (ties and misses by index), in ascending order.  Chosen from the flat scan alone: no tree and no walk has a say."""
    keep = np.argsort(-reaches(name), kind="stable")[:1024]
    keep.sort()
    keep.setflags(write=False)
    return keep


# ------------------------------------------------------------------------------------------ trees and mutants

def median_topology(cen, rad, leaf=4):
    """(topology for bvh_check.assemble, always-tested list): the spheres off the list split at the median of their centres along
    the axis of the largest extent (ties by index) until at most `leaf` are left."""
    always = always_list(cen, rad)
    rest = np.setdiff1d(np.arange(len(rad)), always)

    def split(idx):
        if len(idx) <= leaf:
            return [int(i) for i in idx]
        c = cen[idx].astype(np.float64)
        axis = int(np.argmax(c.max(0) - c.min(0)))
        order = idx[np.argsort(c[:, axis], kind="stable")]
        return (split(order[:len(order) // 2]), split(order[len(order) // 2:]))

    return split(rest), [int(i) for i in always]


@functools.lru_cache(maxsize=None)
def median_tree(name: str):
    """The set's world as a median-split tree that check_bvh has validated: (nodes, recs, ids, info)."""
    arr, _, _ = ray_set(name)
    cen, rad = rq.world_arrays(arr)
    topology, always = median_topology(cen, rad)
    tree = assemble(topology, cen, rad, always)
    check_bvh(*tree, cen, rad)
    return tree


# name -> keyword arguments of bvh_walk_ref.walk.  "kernel" is the walk nearest_hit_bvh performs; everything else is a walk it does not.
MUTANTS = {"kernel": {}, "E = 0": dict(e_scale=0.0), "slack = 1": dict(slack=1.0), "no 2 r_max": dict(cone_rmax=False),
           "E = 0, slack = 1": dict(e_scale=0.0, slack=1.0)}
for _k in range(1, 9):
    MUTANTS[f"E / 2^{_k}"] = dict(e_scale=float(E_SCALE) * 2.0 ** -_k)


def walk_tree(tree, name: str, mutant: str = "kernel", subset=None) -> np.ndarray:
    """The records the (mutant) numpy walk returns for the set's rays, or `subset` of them, on `tree` = (nodes, recs, ids, info)."""
    arr, o, d = ray_set(name)
    if subset is not None:
        o, d = o[subset], d[subset]
    depth = max(int(tree[3]["plan"]["max_depth"]), 1)
    got, _, dropped = walk(*tree, o, d, T_MAX, depth, rq.world_arrays(arr)[1], **MUTANTS[mutant])
    assert dropped.sum() == 0
    return got


@functools.lru_cache(maxsize=None)
def median_walk(name: str, mutant: str = "kernel") -> np.ndarray:
    """walk_tree on the set's median tree, computed once per (set, mutant)."""
    got = walk_tree(median_tree(name), name, mutant)
    got.setflags(write=False)
    return got


def changed(a: np.ndarray, b: np.ndarray) -> int:
    return int((~rq.same_bits(a, b)).sum())
