"""Worlds whose BVH is 20 to 32 levels deep, and ray sets that fill the traversal stack of such a tree to its last entry (host-side
data only; a helper like hbm_worlds.py, not a conftest).

The "line" worlds: K groups of M = 5 spheres, group k near x_k = 2^(top - k) on the x axis, jittered by +-5 % of x_k along x and
laterally, every radius 2^-5 x_min (x_min = 2^(top - K + 1): the innermost group's place).  Equal radii keep every sphere off the
always-tested list.  The host builder's binned SAH peels the outer groups level by level (about 2.2 octaves per level), so the tree
is a caterpillar whose deep end is the dense end.  A ray that starts just beyond the dense end (x = -4 x_min) and heads towards +x
at a small slope meets, at every level, the deep child first and pushes the shallow one: at the deepest leaf the stack holds one
entry per level.

Where the line sits.  The innermost spheres must be HIT for a stack that is one entry short to change an answer (the push that does
not fit is the deepest one: the sibling of the deepest leaf), and test_sphere computes disc = b^2 - a (|oc|^2 - r^2), which is about
|d|^2 r^2 for a central hit, in float32.  With |oc| = 5 x_min, r = 2^-5 x_min and a root above MIN_T = 2^-10 (|d| < 5 x 2^10 x_min)
disc is at most 25 x 2^10 x_min^4: for x_min = 2^-55, 2^-205 -- it underflows to zero, and no float32 ray can hit the inner
groups wherever it starts.  x_min = 2^-24 keeps disc near 2^-94 for directions of length 16 x_min, and the outer end of the
80-octave line32 at 2^55, whose squares (2^110) and the builder's area x count products (about 2^116) stay finite.  Scaling by a
power of two changes no rounding, so the trees have the shape they have anywhere else on the exponent axis where nothing
underflows.

The three-axis staircase is the world for the device builder: a single axis separates only 13 Morton levels, three axes 39, and the
builder's depth rule then holds the tree at MIRT_BVH_MAX_DEPTH = 32.  Its rays start 300 world extents away: from there the 2^-8 L
slack of bvh_slab exceeds the world, every box is a visit, and equal entry parameters send the walk to the left (low Morton codes:
the corner at the origin, the deep end) first.
"""
from __future__ import annotations

import functools

import numpy as np

from hbm_worlds import sphere_array

f32 = np.float32
M = 5                       # spheres per group
X_MIN_LOG2 = -24            # the innermost group of every line world sits at 2^-24
T_MAX = f32(1.0e30)         # the bound of the ray sets: beyond every sphere (t <= 2^57 / 2^-20 = 2^77), finite

# name -> (K, seed): seeds chosen so that the audit of tests/test_deep_trees_cpu.py passes on the host builder's tree
LINES = {"line22": (48, 3), "line24": (52, 5), "line26": (60, 5), "line32": (80, 2)}
# name -> (lowest, highest host max_depth the world is made for)
TARGETS = {"line22": (20, 22), "line24": (23, 25), "line26": (26, 31), "line32": (32, 32)}


def pool_geometry(depth: int):
    """(slots, waves per CU) of the pooled kernel on a tree `depth` deep, written out from the byte formula of include/mirt.h: 16
    waves with 112 slots up to depth 16, 96 to 19, 80 to 22, 64 to 25; beyond that three blocks (12 waves) are the most that fit,
    with 112 slots up to depth 29 and 96 from 30 to 32."""
    for top, geometry in ((16, (112, 16)), (19, (96, 16)), (22, (80, 16)), (25, (64, 16)), (29, (112, 12)), (32, (96, 12))):
        if depth <= top:
            return geometry
    raise ValueError(depth)


def x_min() -> float:
    return 2.0 ** X_MIN_LOG2


def line_world(K: int, seed: int) -> np.ndarray:
    """K groups of M spheres (SPHERE_DTYPE), group 0 the outermost: sphere index = M * k + j."""
    rng = np.random.default_rng(seed)
    top = X_MIN_LOG2 + K - 1
    xk = 2.0 ** (top - np.arange(K, dtype=np.float64))
    jit = rng.uniform(-0.05, 0.05, (K, M, 3))
    cen = jit * xk[:, None, None]
    cen[:, :, 0] += xk[:, None]
    rad = np.full(K * M, 2.0 ** -5 * x_min())
    return sphere_array(cen.reshape(-1, 3), rad, np.arange(K * M) % 7)


@functools.lru_cache(maxsize=None)
def line(name: str) -> np.ndarray:
    return line_world(*LINES[name])            # (writable: ctypes views of it are taken; nobody writes)


def line_rays(arr: np.ndarray, seed: int = 0, n: int = 4096, inner_groups: int = 6):
    """(origins, directions) float32 [n, 3] for a line world.  First half, from beyond the dense end (x = -4 x_min, a little off the
    axis): three quarters aimed at the spheres of the innermost groups (round-robin, the aim point within 1.5 radii of the centre:
    hits and near misses), the rest at small random slopes.  Second half: the same lines from beyond the sparse end, heading
    towards -x.  Directions are 16 x_min long."""
    rng = np.random.default_rng(seed)
    cen = arr["center"][:, :3].astype(np.float64)
    r = float(arr["radius"][0])
    xm = x_min()
    half = n // 2
    n_aim = half * 3 // 4
    o = np.zeros((half, 3))
    o[:, 0] = -4.0 * xm
    o[:, 1:] = rng.uniform(-0.02, 0.02, (half, 2)) * xm
    inner = np.arange(len(arr) - inner_groups * M, len(arr))
    target = cen[inner[np.arange(n_aim) % len(inner)]] + rng.uniform(-1.5, 1.5, (n_aim, 3)) * r / np.sqrt(3.0)
    d = np.empty((half, 3))
    d[:n_aim] = target - o[:n_aim]
    slope = rng.uniform(-0.06, 0.06, (half - n_aim, 2))
    d[n_aim:] = np.concatenate([np.ones((half - n_aim, 1)), slope], 1)
    d *= (16.0 * xm / np.linalg.norm(d, axis=1))[:, None]
    # the same lines from x = 4 x_max
    s = (4.0 * cen[:, 0].max() - o[:, 0]) / d[:, 0]
    o2, d2 = o + s[:, None] * d, -d
    return np.concatenate([o, o2]).astype(f32), np.concatenate([d, d2]).astype(f32)


@functools.lru_cache(maxsize=None)
def line_set(name: str):
    """(world, origins, directions) of a line world's ray set; read-only, shared."""
    arr = line(name)
    o, d = line_rays(arr)
    o.setflags(write=False)
    d.setflags(write=False)
    return arr, o, d


def line_camera(w: int, h: int):
    """A camera at the dense end of a line world looking along +x: the innermost groups fill the frame."""
    from hbm_worlds import look
    xm = x_min()
    return look(w, h, (-4.0 * xm, 0.01 * xm, 0.005 * xm), (xm, 0.0, 0.0), vfov=2.5, focus=16.0 * xm)


# ------------------------------------------------------------------------------------------ a hand-made caterpillar

CATERPILLAR_K = 26          # 130 spheres: 32 side leaves of 4 and a last leaf of 2


def caterpillar(seed=6):
    """(world, topology): a line world of 26 groups and the nested-pair topology (bvh_check.assemble) of a 32-level caterpillar over
    it: every inner node has a leaf of 4 spheres and the rest of the line; the two spheres left at the end are the last leaf, at
    depth 32 like its sibling.  A side leaf takes the outermost sphere not yet placed and three of the next eight such that the
    leaf's box straddles the x axis by 2 % of its nearest sphere's distance in y and in z: a ray along the line crosses every one
    of them (four spheres taken in plain x order leave the axis outside their box at one level in four).  Not every seed allows
    it; 6 does."""
    import itertools
    arr = line_world(CATERPILLAR_K, seed)
    cen = arr["center"][:, :3].astype(np.float64)
    left = [int(i) for i in np.argsort(-cen[:, 0], kind="stable")]
    side = []
    for _ in range(32):
        head, pool = left[0], left[1:9]
        for trio in itertools.combinations(pool, 3):
            c = cen[[head, *trio]]
            m = 0.02 * c[:, 0].min()
            if (c[:, 1:].min(0) < -m).all() and (c[:, 1:].max(0) > m).all():
                break
        else:
            raise AssertionError("no straddling leaf: choose another seed")
        side.append([head, *trio])
        left = [i for i in left if i not in side[-1]]
    t = left
    assert len(t) == 2
    for leaf in reversed(side):
        t = (leaf, t)
    return arr, t


def caterpillar_rays(arr: np.ndarray):
    """The line set of the caterpillar's world with the aimed rays on its innermost 8 spheres: the last leaf and its sibling."""
    return line_rays(arr, seed=1, inner_groups=2)


# ------------------------------------------------------------------------------------------ the device builder's world

STAIR_RADIUS = 2.0 ** -4


def axes_staircase(steps: int = 24, seed: int = 15) -> np.ndarray:
    """For k = 1 .. steps and each axis a, five centres within 2^-(k+4) (towards + + +) of 2^-k e_a, and five next to the origin:
    three at (0, 0, 2^-11) and two at (0, 2^-11, 0).  The centroid box starts at 0, so group k on axis a keeps the top bit of its
    cell to itself: Morton splits peel one group per level (3 x steps levels) until the depth rule takes over, at depth 32; the last
    five split 3 | 2 (y's code bit stands above z's), one level further down.
    Every radius is 2^-4 (nothing goes to the always-tested list): the spheres overlap, a ray from the (-, -, -) octant that
    passes the origin hits in earnest, and the nearest surface along it belongs to the last five.  Their two boxes differ in y and
    z only: a ray that enters both through the x slab enters them at the same parameter, goes LEFT first and pushes the right
    leaf -- the push a stack one entry short drops -- and where its direction has more z than y the right leaf's spheres are the
    nearer ones."""
    rng = np.random.default_rng(seed)
    cen = []
    for k in range(1, steps + 1):
        for a in range(3):
            base = np.zeros(3)
            base[a] = 2.0 ** -k
            cen.append(base + rng.uniform(0, 1, (5, 3)) * 2.0 ** -(k + 4))
    c = 2.0 ** -11
    cen = np.concatenate(cen + [np.array([[0, 0, c]] * 3 + [[0, c, 0]] * 2)])
    return sphere_array(cen, np.full(len(cen), STAIR_RADIUS), np.arange(len(cen)) % 7)


STAIR_EXTENT = 0.5 + 2.0 ** -5


# name -> steps: the device builder's tree is 3 x steps + 1 deep until its depth rule stops it at 32
STAIRS = {"stair22": 7, "stair25": 8, "stair28": 9, "stair32": 24}
# The depths both builders give every world.  The host's are mirt_bvh_plan's (tests/test_deep_trees_cpu.py holds them to it); the
# device's were first replayed in numpy from the builder's description (13-bit cubic cells, Morton order, the depth rule) to make
# the worlds, and tests/test_gpu_deep_trees.py holds the trees read back from the device to them.
HOST_DEPTH = {"line22": 22, "line24": 25, "line26": 26, "line32": 32, "stair22": 8, "stair25": 9, "stair28": 10, "stair32": 22}
DEVICE_DEPTH = {"line22": 19, "line24": 20, "line26": 20, "line32": 20, "stair22": 22, "stair25": 25, "stair28": 28, "stair32": 32}


@functools.lru_cache(maxsize=None)
def stair(name: str) -> np.ndarray:
    return axes_staircase(STAIRS[name])


def staircase_rays(arr: np.ndarray, seed: int = 2, n: int = 4096):
    """(origins, directions): origins 300 world extents from the origin in the (-, -, -) octant, aimed at points of the world's box;
    a hit from there is rounding's doing (a sphere of radius 2^-30 seen from 160 units), which the flat scan and the walk must
    agree on.  The last quarter starts next to the origin's group instead, where spheres are hit in earnest."""
    rng = np.random.default_rng(seed)
    far = n - n // 4
    u = rng.uniform(0.6, 1.0, (far, 3))
    o = -300.0 * STAIR_EXTENT * u / np.linalg.norm(u, axis=1)[:, None]
    at = rng.uniform(0.0, 1.0, (far, 3)) ** 4 * STAIR_EXTENT
    d = at - o
    d *= (rng.uniform(0.5, 2.0, far) / np.linalg.norm(d, axis=1))[:, None]
    cen = arr["center"][:, :3].astype(np.float64)
    near = n // 4
    o2 = -rng.uniform(0.5, 1.0, (near, 3)) * 2.0 ** -26
    tgt = cen[rng.integers(0, len(cen), near)] + rng.uniform(-1, 1, (near, 3)) * 2.0 ** -30
    d2 = tgt - o2
    d2 *= (2.0 ** -27 / np.linalg.norm(d2, axis=1))[:, None]
    return np.concatenate([o, o2]).astype(f32), np.concatenate([d, d2]).astype(f32)


def staircase_camera(w: int, h: int):
    """300 extents away in the (-, -, -) octant, looking at the origin with a frame 0.06 wide there: every primary ray passes the
    last five spheres (radius 2^-4).  The view direction (1, 0.3, 0.9) has most x and much more z than y: the rays enter the last
    two leaves through the x slab, at equal parameters, so the walk goes left and pushes the right leaf, whose spheres are the
    nearer ones by 2^-11 x 0.43.  That is a few units in the last place of a root computed 160 units away: on a good part of the
    pixels (69 to 474 of 1 536, by the numpy walk) the winner is one of the right leaf, and a stack one entry short changes what
    the camera sees.  Direction and width were chosen for that count; (1, 0.5, 0.9) leaves 1 such pixel on two of the worlds."""
    from hbm_worlds import look
    dist = 300.0 * STAIR_EXTENT
    u = np.array([1.0, 0.3, 0.9])
    eye = -dist * u / np.linalg.norm(u)
    return look(w, h, eye, (0.0, 0.0, 0.0), vfov=float(np.degrees(2 * np.arctan(0.03 / dist))), focus=1.0)


# ------------------------------------------------------------------------------------------ sets by name, references computed once

@functools.lru_cache(maxsize=None)
def ray_set(name: str):
    """(world, origins, directions) of "line22" .. "line32", "stair22" .. "stair32" or "caterpillar"; the rays read-only."""
    if name in LINES:
        return line_set(name)
    if name in STAIRS:
        arr = stair(name)
        o, d = staircase_rays(arr)
    elif name == "caterpillar":
        arr, _ = caterpillar()
        o, d = caterpillar_rays(arr)
    else:
        raise KeyError(name)
    for a in (o, d):
        a.setflags(write=False)
    return arr, o, d


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    """ray_query_ref.trace_ref of a set under T_MAX: the flat scan's records, shared by every test that needs them."""
    import ray_query_ref as rq
    arr, o, d = ray_set(name)
    ref = rq.trace_ref(o, d, T_MAX, *rq.world_arrays(arr))
    ref.setflags(write=False)
    return ref


def line_camera_long(arr: np.ndarray, w: int, h: int):
    """The same eye and view with primary rays x_max / 64 long: every group lies within t < 1000 (kMaxT), so a render kernel's walk
    -- whose bound is fixed -- visits both children at every level and fills its stack, which under line_camera it cannot (1000
    directions of 16 x_min end 14 octaves up the line).  What such rays can hit lies 2^-10 of their length away and beyond: the
    outer groups, by rounding alone."""
    from hbm_worlds import look
    xm = x_min()
    return look(w, h, (-4.0 * xm, 0.01 * xm, 0.005 * xm), (xm, 0.0, 0.0), vfov=2.5, focus=float(arr["center"][:, 0].max()) / 64.0)
