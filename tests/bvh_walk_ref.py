"""nearest_hit_bvh (csrc/mirt_kernels.hip) restated in numpy, for a tree as Context.bvh_read() / bvh_info() return it: an auditing
tool that tells how full the traversal stack gets and what a stack of another size would have answered.

The walk is the kernel's, operation for operation in float32: the always-tested list first, then near child first with the (tn, tf)
of bvh_slab -- the exact build compiles with -ffp-contract=off, so the slab arithmetic is plain rounded products and sums; fma32
stands only where the kernel calls fma_ (the dot products) -- the bound e = min(e_box, e_cone) with grow() after every leaf, the
three negated comparisons with kBvhSlack, and the push dropped when sp == stack_cap.  Sphere tests are grid_rounding.first_roots
on the tree's own records, a tie going to the lower original id.  All rays advance together, one node per ray and pass, as the
lanes of a wave do.

It has to agree with the device on WINNERS (which are the flat scan's whatever is visited); a visit decided by the last bit of a
comparison may differ without consequence.  Host-side only; a helper like ray_query_ref.py, not a conftest."""
from __future__ import annotations

import numpy as np

from bvh_check import LEAF
from grid_rounding import dot32, first_roots_rr
import ray_query_ref as rq

f32 = np.float32
SLACK = f32(1.0) + f32(2.0 ** -9)                 # kBvhSlack
E_SCALE = f32(f32(2.0 ** -8) * f32(1.01))         # 0x1p-8f * 1.01f


def _slab(lo, hi, ro, inv, sgn, e_cone, e_scale=E_SCALE):
    """bvh_slab for boxes (lo, hi) [k, 3] and rays (ro, inv, sgn) [k, 3], e_cone [k] -> (tn, tf).  `e_scale` stands for the kernel's
    0x1p-8f * 1.01f in the farthest-corner bound."""
    d = np.maximum(np.abs(lo - ro), np.abs(hi - ro))
    e_box = f32(e_scale) * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    e = np.where(e_box < e_cone, e_box, e_cone)
    ev = e[:, None] * np.abs(inv)
    near = (np.where(sgn, lo, hi) - ro) * inv - ev
    far = (np.where(sgn, hi, lo) - ro) * inv + ev
    tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2])
    tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
    return tn, tf


def walk(nodes, recs, ids, info, o, d, t_max, stack_cap, radii=None, e_scale=E_SCALE, slack=SLACK, cone_rmax=True):
    """-> (hits RAY_HIT_DTYPE [n], high water [n], dropped pushes [n]) of rays (o, d) [n, 3] bounded by t_max (scalar or [n]) on the
    tree (nodes, recs, ids, info) with a stack of `stack_cap` entries.  `radii` [n_spheres] in original order give the hit records
    their normals; None: the square roots of the records' r * r (exact for the power-of-two radii of the deep worlds).

    The slack of the walk as parameters, the kernel's values the defaults -- anything else is a MUTANT, a walk the kernel does not
    perform, for showing that a set of rays needs the slack (tests/test_bvh_rounding_cpu.py): `e_scale` replaces 0x1p-8f * 1.01f in
    all three bounds of E (0: boxes are not grown), `slack` replaces kBvhSlack in both comparisons that carry it, and
    cone_rmax=False drops the 2 r_max term of the cone bound."""
    e_scale, slack = f32(e_scale), f32(slack)
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    n = len(o)
    recs = np.asarray(recs, f32).reshape(-1, 4)
    ids = np.asarray(ids).astype(np.int64)
    n_always = int(info["plan"]["n_always"])
    t_max = np.broadcast_to(np.asarray(t_max, f32), (n,))
    with np.errstate(all="ignore"):
        F = np.concatenate([first_roots_rr(o[i:i + 512], d[i:i + 512], recs[:, :3], recs[:, 3]) for i in range(0, n, 512)]) \
            if n and len(recs) else np.zeros((n, len(recs)), f32)
        closest = t_max.astype(f32).copy()
        best = np.full(n, -1, np.int64)
        best_f = np.full(n, np.inf, f32)

        def take(rays, rec):
            f, i = F[rays, rec], ids[rec]
            t = np.isfinite(f) & ((f < closest[rays]) | ((f == closest[rays]) & (i < best[rays])))
            r = rays[t]
            closest[r], best[r], best_f[r] = f[t], i[t], f[t]

        everyone = np.arange(n)
        for j in range(n_always):
            take(everyone, np.full(n, j))

        a = dot32(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
        inv = (f32(1.0) / d).astype(f32)
        sgn = inv >= 0
        dc = (o - np.asarray(info["centre"], f32)).astype(f32)
        e_world = e_scale * (np.sqrt(dot32(dc[:, 0], dc[:, 1], dc[:, 2], dc[:, 0], dc[:, 1], dc[:, 2])) + f32(info["radius"]))
        len_d = f32(1.01) * np.sqrt(a)
        two_rmax = f32(2.0) * f32(info["r_max"]) if cone_rmax else f32(0.0)

        def grow(rays):
            e = e_scale * (closest[rays] * len_d[rays] + two_rmax)
            return np.where(e < e_world[rays], e, e_world[rays])

        e_cone = grow(everyone)
        ref = np.full(n, int(info["root"]), np.int64)
        sp = np.zeros(n, np.int64)
        stack = np.zeros((n, max(int(stack_cap), 1)), np.int64)
        high = np.zeros(n, np.int64)
        dropped = np.zeros(n, np.int64)
        go = np.ones(n, bool)
        while go.any():
            act = np.nonzero(go)[0]
            is_leaf = (ref[act] & LEAF) != 0
            pop = np.zeros(n, bool)
            lv = act[is_leaf]
            if len(lv):
                first, cnt = ref[lv] & 0xffffff, (ref[lv] >> 24) & 0x7f
                for k in range(int(cnt.max(initial=0))):
                    m = cnt > k
                    take(lv[m], first[m] + k)
                e_cone[lv] = grow(lv)
                pop[lv] = True
            iv = act[~is_leaf]
            if len(iv):
                nd = nodes[ref[iv]]
                ro, ri, sg, ec = o[iv], inv[iv], sgn[iv], e_cone[iv]
                tnl, tfl = _slab(nd["lmin"], nd["lmax"], ro, ri, sg, ec, e_scale)
                tnr, tfr = _slab(nd["rmin"], nd["rmax"], ro, ri, sg, ec, e_scale)
                lim = closest[iv] * slack
                vl = ~(tnl > lim) & ~(tfl < 0) & ~(tnl > tfl * slack)
                vr = ~(tnr > lim) & ~(tfr < 0) & ~(tnr > tfr * slack)
                lref, rref = nd["left"].astype(np.int64), nd["right"].astype(np.int64)
                both, one = vl & vr, vl ^ vr
                left_first = ~(tnr < tnl)
                ref[iv] = np.where(both, np.where(left_first, lref, rref), np.where(vl, lref, rref))
                pb = iv[both]
                fits = sp[pb] < stack_cap
                pf = pb[fits]
                stack[pf, sp[pf]] = np.where(left_first, rref, lref)[both][fits]
                sp[pf] += 1
                dropped[pb[~fits]] += 1
                high[pf] = np.maximum(high[pf], sp[pf])
                pop[iv[~both & ~one]] = True
            pv = np.nonzero(pop)[0]
            done = pv[sp[pv] == 0]
            go[done] = False
            more = pv[sp[pv] > 0]
            sp[more] -= 1
            ref[more] = stack[more, sp[more]]

    # the record of the winner, by the reference's own resolve: a roots matrix that holds the winner's root alone
    n_spheres = len(ids)
    f = np.full((n, max(n_spheres, 1)), np.inf, f32)
    won = best >= 0
    f[np.nonzero(won)[0], best[won]] = best_f[won]
    cen = np.zeros((max(n_spheres, 1), 3), f32)
    rad = np.ones(max(n_spheres, 1), f32)
    if n_spheres:
        cen[ids] = recs[:, :3]
        rad[ids] = np.sqrt(recs[:, 3])
        if radii is not None:
            rad = np.asarray(radii, f32)
    return rq.resolve(f, o, d, t_max, cen, rad), high, dropped
