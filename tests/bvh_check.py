"""A validator of a BVH as a MIRT_SCENE_HBM context holds it (Context.bvh_read / bvh_info), in numpy, for either builder.

The image of such a scene is the flat scan's whatever the tree's shape as long as the properties checked here
hold: every sphere that is not on the always-tested list sits in exactly one leaf, the list is the host rule's, the records are
{centre, r * r} of their spheres, leaves hold at most 4 spheres, no leaf lies deeper than 32, every child box EQUALS the union of the
outward-rounded boxes of the spheres below it, and centre / radius / r_max bound the boxes and the radii.  `check_bvh` raises
BvhError with the first violation.  No GPU, no library: the formulas are written out again here.  `assemble` builds such a tree by
hand from a nested topology, with the validator's own boxes.
"""
from __future__ import annotations

import numpy as np

LEAF = 0x80000000
MAX_LEAF, MAX_DEPTH, MAX_ALWAYS, BIG_RADII = 4, 32, 64, 4

NODE_DTYPE = np.dtype([("lmin", "<f4", (3,)), ("lmax", "<f4", (3,)), ("rmin", "<f4", (3,)), ("rmax", "<f4", (3,)),
                       ("left", "<u4"), ("right", "<u4"), ("pad", "<u4", (2,))])


class BvhError(AssertionError):
    pass


def _need(ok, msg):
    if not ok:
        raise BvhError(msg)


def always_list(centres: np.ndarray, radii: np.ndarray) -> np.ndarray:
    """The host rule (include/mirt.h): spheres whose box is not finite, in index order, up to 64; then the largest above 4 median
    radii, ties to the lower index; the whole list sorted by index.  centres float32 [n, 3], radii float32 [n]."""
    c = centres.astype(np.float64)
    r = np.abs(radii.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(r) & np.all(np.isfinite(c) & np.isfinite(c - r[:, None]) & np.isfinite(c + r[:, None]) & (np.abs(c) + r[:, None] < 3.0e38), axis=1)
    bad = np.flatnonzero(~ok)
    out = list(bad[:MAX_ALWAYS])
    fin = np.flatnonzero(ok)
    if len(fin) and len(out) < MAX_ALWAYS:
        rf = np.abs(radii[fin])                                    # float32, as the host sorts them
        median = np.partition(rf, len(rf) // 2)[len(rf) // 2]
        big = fin[np.abs(radii[fin].astype(np.float64)) > BIG_RADII * float(median)]
        order = sorted(big, key=lambda i: (-abs(float(radii[i])), int(i)))
        out += order[:MAX_ALWAYS - len(out)]
    return np.array(sorted(int(i) for i in out), np.int64)


def _down(v: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    bump = f.astype(np.float64) > v
    f[bump] = np.nextafter(f[bump], np.float32(-np.inf))
    return f


def _up(v: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    bump = f.astype(np.float64) < v
    f[bump] = np.nextafter(f[bump], np.float32(np.inf))
    return f


def sphere_boxes(centres: np.ndarray, radii: np.ndarray):
    """(lo, hi) float32 [n, 3]: lo = down(c - |r| - 2^-20 (|c| + |r|)), hi = up(c + |r| + 2^-20 (|c| + |r|)) in float64, rounded to
    float outwards; a sphere whose centre or radius is not finite: an infinite box."""
    c = centres.astype(np.float64)
    r = np.abs(radii.astype(np.float64))[:, None]
    finite = np.isfinite(r[:, 0]) & np.all(np.isfinite(c), axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        pad = 2.0 ** -20 * (np.abs(c) + r)
        lo = _down(np.where(finite[:, None], c - r - pad, 0.0))
        hi = _up(np.where(finite[:, None], c + r + pad, 0.0))
    lo[~finite] = -np.inf
    hi[~finite] = np.inf
    return lo, hi


def check_bvh(nodes: np.ndarray, recs: np.ndarray, ids: np.ndarray, info: dict, centres: np.ndarray, radii: np.ndarray) -> dict:
    """Raises BvhError at the first violated property; returns the counts of the walk (the MirtBvhPlan fields)."""
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    radii = np.asarray(radii, np.float32).reshape(-1)
    n = len(radii)
    plan = info["plan"]
    n_always = int(plan["n_always"])
    recs = np.asarray(recs, np.float32).reshape(-1, 4)
    ids = np.asarray(ids).astype(np.int64)
    _need(len(ids) == n and len(recs) == n, f"{len(ids)} ids / {len(recs)} records for {n} spheres")
    _need(np.all((ids >= 0) & (ids < n)), "an id is out of range")
    want_always = always_list(centres, radii)
    _need(np.array_equal(ids[:n_always], want_always), f"always-tested list {ids[:n_always].tolist()} != the host rule's {want_always.tolist()}")
    with np.errstate(over="ignore", invalid="ignore"):
        want_recs = np.concatenate([centres[ids], (radii[ids] * radii[ids])[:, None]], axis=1)      # float32 product, as PreparedSphere.rr
    _need(np.array_equal(recs.view(np.uint32), want_recs.view(np.uint32)), "a record is not {centre, r * r} of its sphere")
    lo, hi = sphere_boxes(centres, radii)

    seen = np.zeros(n, np.int64)
    seen[ids[:n_always]] += 1
    count = {"n_nodes": 0, "n_leaves": 0, "n_leaf_spheres": 0, "n_always": n_always, "max_depth": 0, "max_leaf": 0}
    visited = np.zeros(len(nodes), bool)
    boxes = {}                                              # child reference -> (lo, hi) of the spheres below it

    def leaf(ref, depth):
        first, cnt = ref & 0xffffff, (ref >> 24) & 0x7f
        _need(cnt <= MAX_LEAF, f"a leaf of {cnt} spheres")
        _need(depth <= MAX_DEPTH, f"a leaf at depth {depth}")
        _need(first >= n_always and first + cnt <= n or cnt == 0, f"leaf records [{first}, {first + cnt}) outside [{n_always}, {n})")
        if cnt:
            count["n_leaves"] += 1
            count["n_leaf_spheres"] += cnt
            count["max_depth"] = max(count["max_depth"], depth)
            count["max_leaf"] = max(count["max_leaf"], cnt)
        j = ids[first:first + cnt]
        seen[j] += 1
        if cnt == 0:
            return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
        return lo[j].min(axis=0), hi[j].max(axis=0)

    root = int(info["root"])
    if root & LEAF:
        _need(len(nodes) == 0, "a leaf root with inner nodes")
        leaf(root, 0)
    else:
        # iterative post-order walk: (node, depth, expanded)
        stack = [(root, 0, False)]
        while stack:
            ref, depth, expanded = stack.pop()
            _need(ref < len(nodes), f"child reference {ref} beyond {len(nodes)} nodes")
            nd = nodes[ref]
            kids = (int(nd["left"]), int(nd["right"]))
            if not expanded:
                _need(not visited[ref], f"node {ref} has two parents")
                visited[ref] = True
                count["n_nodes"] += 1
                _need(depth < MAX_DEPTH, f"an inner node at depth {depth}")
                stack.append((ref, depth, True))
                for side, k in enumerate(kids):
                    if k & LEAF:
                        boxes[(ref, side)] = leaf(k, depth + 1)
                    else:
                        stack.append((k, depth + 1, False))
                continue
            for side, (k, (kl, kh)) in enumerate(zip(kids, (("lmin", "lmax"), ("rmin", "rmax")))):
                want = boxes.pop((ref, side)) if k & LEAF else boxes.pop(k)
                got = (nd[kl], nd[kh])
                _need(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]),
                      f"node {ref}: box of child {k:#x} is {got[0].tolist()} .. {got[1].tolist()}, the union below it {want[0].tolist()} .. {want[1].tolist()}")
            boxes[ref] = (np.minimum(nd["lmin"], nd["rmin"]), np.maximum(nd["lmax"], nd["rmax"]))
        _need(visited.all(), f"{int((~visited).sum())} nodes are not reachable from the root")
    if n:
        _need(np.all(seen >= 1), f"sphere {int(np.argmin(seen))} is in no leaf")
        _need(np.all(seen <= 1), f"sphere {int(np.argmax(seen))} is tested {int(seen.max())} times")
    for k, v in count.items():
        _need(int(plan[k]) == v, f"info.plan.{k} = {plan[k]}, the walk finds {v}")
    _need(int(plan["device_bytes"]) == 64 * count["n_nodes"] + 20 * n, "info.plan.device_bytes")

    # the traversal bounds: a sphere of `radius` around `centre` holds every tree box, r_max every tree radius (3.0e38 stands for "unbounded")
    tree = np.ones(n, bool)
    tree[ids[:n_always]] = False
    if tree.any():
        cen = np.asarray(info["centre"], np.float64)
        radius, r_max = float(info["radius"]), float(info["r_max"])
        tl, th = lo[tree].astype(np.float64), hi[tree].astype(np.float64)
        fin = np.all(np.isfinite(tl) & np.isfinite(th), axis=1)
        if fin.any():
            with np.errstate(over="ignore", invalid="ignore"):
                far = np.sqrt((np.maximum(np.abs(tl[fin] - cen), np.abs(th[fin] - cen)) ** 2).sum(axis=1)).max()
            _need(radius >= min(far, 3.0e38), f"radius {radius} < the farthest box corner {far}")
            if not fin.all():
                _need(radius >= np.float32(3.0e38), f"radius {radius} with an infinite box in the tree")
            rr = np.abs(radii[tree].astype(np.float64))
            rr = rr[~np.isnan(rr)]
            if len(rr):
                _need(r_max >= min(rr.max(), 3.0e38), f"r_max {r_max} < the largest radius {rr.max()}")
    return count


def assemble(topology, centres, radii, always=()):
    """(nodes, recs, ids, info) of a tree given as nested pairs whose leaves are lists of sphere indices; boxes by the validator's own
    per-sphere formula, so that a test changes exactly one thing afterwards."""
    centres = np.asarray(centres, np.float32)
    radii = np.asarray(radii, np.float32)
    lo, hi = sphere_boxes(centres, radii)
    ids = [int(i) for i in always]
    nodes = []
    stat = {"n_leaves": 0, "max_depth": 0, "max_leaf": 0}

    def build(t, depth):
        """-> (reference, lo, hi)"""
        if isinstance(t, list):
            ref = LEAF | (len(t) << 24) | len(ids)
            ids.extend(t)
            if t:
                stat["n_leaves"] += 1
                stat["max_depth"] = max(stat["max_depth"], depth)
                stat["max_leaf"] = max(stat["max_leaf"], len(t))
            if not t:
                return ref, np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
            return ref, lo[t].min(axis=0), hi[t].max(axis=0)
        me = len(nodes)
        nodes.append(None)
        l, r = build(t[0], depth + 1), build(t[1], depth + 1)
        nd = np.zeros((), NODE_DTYPE)
        nd["left"], nd["lmin"], nd["lmax"] = l
        nd["right"], nd["rmin"], nd["rmax"] = r
        nodes[me] = nd
        return me, np.minimum(l[1], r[1]), np.maximum(l[2], r[2])

    root, blo, bhi = build(topology, 0)
    ids = np.array(ids, np.uint32)
    recs = np.concatenate([centres[ids], (radii[ids] * radii[ids])[:, None]], axis=1).astype(np.float32)
    if not len(ids) - len(always):                       # an empty tree: there is nothing to bound
        blo, bhi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    cen = (0.5 * (blo.astype(np.float64) + bhi)).astype(np.float32)
    far = np.sqrt((np.maximum(np.abs(blo - cen.astype(np.float64)), np.abs(bhi - cen.astype(np.float64))) ** 2).sum())
    info = {"plan": {"n_nodes": len(nodes), "n_leaves": stat["n_leaves"], "n_leaf_spheres": len(ids) - len(always), "n_always": len(always),
                     "max_depth": stat["max_depth"], "max_leaf": stat["max_leaf"], "device_bytes": 64 * len(nodes) + 20 * len(ids)},
            "root": root, "built_on_device": 0, "centre": cen.tolist(), "radius": float(np.float32(far * 1.001)),
            "r_max": float(np.float32(np.nanmax(np.abs(radii[ids[len(always):]]), initial=0.0) * 1.001))}
    return np.array(nodes, NODE_DTYPE) if nodes else np.zeros(0, NODE_DTYPE), recs, ids, info
