// mirt_bvh.cpp — host BVH builder of MIRT_SCENE_HBM scenes (include/mirt.h: mirt_ctx_set_scene_ex, mirt_bvh_plan).
//
// Binned SAH over the sphere centres (16 bins on the centroid box's longest axis), binary, leaves of at most MIRT_BVH_MAX_LEAF
// spheres.  Boxes use |radius| (a negative radius -- the hollow-glass idiom -- is valid input) and are rounded outwards.  Up to
// MIRT_BVH_MAX_ALWAYS spheres go to an always-tested list instead of the tree: those whose box is not finite, then the largest of
// those above MIRT_BVH_BIG_RADII median radii (a ground sphere would otherwise sit in the root's boxes and defeat every split).
//
// Depth is bounded BY CONSTRUCTION: a subtree of m spheres built by object-median splits is ceil(log2(ceil(m / 4))) levels deep.  A
// node at depth d takes its SAH split only if both children could still be finished that way within MIRT_BVH_MAX_DEPTH
// (d + 1 + ceil(log2(ceil(m / 4))) <= MIRT_BVH_MAX_DEPTH), else it splits at the median (by centre, ties by index).  The root
// satisfies the rule for every n <= 2^24 (22 levels), and a median split keeps it, so no leaf lies deeper than the limit -- not even
// for 10 000 identical spheres, where every split is a median split.
//
// Single-threaded (well within the 16-thread budget of the host side), deterministic: the same spheres give the same tree, byte for
// byte (std::partition / std::nth_element with an index tie-break are pure functions of their input).
#include "mirt_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace mirt {
int set_error(int status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // mirt_api.hip
}

namespace {

struct Box {
    double lo[3], hi[3];
    void clear() { for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; } }
    void grow(const Box& b) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); } }
    void grow(const double p[3]) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); } }
    double area() const
    {
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return (dx < 0 || dy < 0 || dz < 0) ? 0.0 : dx * dy + dy * dz + dz * dx;
    }
};

uint32_t ceil_log2(uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; }
// levels a subtree of m spheres needs when every split is a median split
uint32_t median_levels(uint64_t m) { return ceil_log2((m + MIRT_BVH_MAX_LEAF - 1) / MIRT_BVH_MAX_LEAF); }

float down(double v) { float f = (float)v; if ((double)f > v) f = std::nextafter(f, -INFINITY); return f; }
float up(double v)   { float f = (float)v; if ((double)f < v) f = std::nextafter(f, INFINITY); return f; }

struct Item {
    Box      box;          // rounded outwards: the float box the kernel tests contains it
    double   c[3];         // centre (binning)
    uint32_t id;
};

constexpr int kBins = 16;

// split [b, e) of `items` (at depth d); returns the first index of the right child
uint32_t split(std::vector<Item>& items, uint32_t b, uint32_t e, uint32_t depth)
{
    const uint32_t n = e - b;
    Box cb; cb.clear();
    for (uint32_t i = b; i < e; ++i) cb.grow(items[i].c);
    int axis = 0;
    for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
    const double lo = cb.lo[axis], ext = cb.hi[axis] - cb.lo[axis];
    auto median = [&]() {
        const uint32_t mid = b + (n + 1) / 2;
        std::nth_element(items.begin() + b, items.begin() + mid, items.begin() + e, [axis](const Item& x, const Item& y) {
            return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.id < y.id);
        });
        return mid;
    };
    if (!(ext > 0.0) || !std::isfinite(ext)) return median();
    auto bin_of = [&](const Item& it) {
        const int k = (int)((it.c[axis] - lo) * (kBins / ext));
        return k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
    };
    Box bb[kBins];
    uint32_t cnt[kBins] = {};
    for (int k = 0; k < kBins; ++k) bb[k].clear();
    for (uint32_t i = b; i < e; ++i) { const int k = bin_of(items[i]); bb[k].grow(items[i].box); cnt[k] += 1; }
    // sweep: cost of the split after bin k = area(left) * n_left + area(right) * n_right
    double right_area[kBins];
    uint32_t right_n[kBins];
    {
        Box acc; acc.clear();
        uint32_t m = 0;
        for (int k = kBins - 1; k >= 1; --k) { acc.grow(bb[k]); m += cnt[k]; right_area[k] = acc.area(); right_n[k] = m; }
    }
    Box acc; acc.clear();
    uint32_t m = 0;
    double best = INFINITY;
    int best_k = -1;
    for (int k = 0; k < kBins - 1; ++k) {
        acc.grow(bb[k]); m += cnt[k];
        if (m == 0 || right_n[k + 1] == 0) continue;
        const double cost = acc.area() * m + right_area[k + 1] * right_n[k + 1];
        if (cost < best) { best = cost; best_k = k; }
    }
    if (best_k < 0) return median();
    uint32_t n_left = 0;
    for (int k = 0; k <= best_k; ++k) n_left += cnt[k];
    // the depth rule (see the top of the file): both children must still fit below MIRT_BVH_MAX_DEPTH with median splits
    if (depth + 1 + median_levels(n_left) > MIRT_BVH_MAX_DEPTH || depth + 1 + median_levels(n - n_left) > MIRT_BVH_MAX_DEPTH) return median();
    const auto it = std::partition(items.begin() + b, items.begin() + e, [&](const Item& x) { return bin_of(x) <= best_k; });
    return (uint32_t)(it - items.begin());
}

}  // namespace

namespace mirt {

std::vector<uint32_t> bvh_always_list(const MirtSphere* s, uint32_t n)
{
    std::vector<uint32_t> bad, finite_ids;             // boxes that are not finite / the rest
    std::vector<float> radii;
    finite_ids.reserve(n);
    radii.reserve(n);
    for (uint32_t i = 0; i < n; ++i) {
        const double r = std::fabs((double)s[i].radius);
        bool ok = std::isfinite(r);
        for (int k = 0; k < 3; ++k) ok = ok && std::isfinite((double)s[i].center[k]) && std::isfinite((double)s[i].center[k] - r) &&
                                           std::isfinite((double)s[i].center[k] + r) && std::fabs((double)s[i].center[k]) + r < 3.0e38;
        if (!ok) { bad.push_back(i); continue; }
        finite_ids.push_back(i);
        radii.push_back(std::fabs(s[i].radius));
    }
    std::vector<uint32_t> always(bad.begin(), bad.begin() + std::min<size_t>(bad.size(), MIRT_BVH_MAX_ALWAYS));
    if (!radii.empty() && always.size() < MIRT_BVH_MAX_ALWAYS) {
        std::nth_element(radii.begin(), radii.begin() + radii.size() / 2, radii.end());        // the median; `radii` is not read again
        const double limit = (double)MIRT_BVH_BIG_RADII * radii[radii.size() / 2];
        std::vector<uint32_t> big;
        for (uint32_t i : finite_ids) if (std::fabs((double)s[i].radius) > limit) big.push_back(i);
        std::sort(big.begin(), big.end(), [s](uint32_t x, uint32_t y) {
            const float rx = std::fabs(s[x].radius), ry = std::fabs(s[y].radius);
            return rx > ry || (rx == ry && x < y);
        });
        for (uint32_t i : big) {
            if (always.size() >= MIRT_BVH_MAX_ALWAYS) break;
            always.push_back(i);
        }
    }
    std::sort(always.begin(), always.end());
    return always;
}

void bvh_round_bounds(double rad, double rmax, float* radius, float* r_max)
{
    *radius = up(rad * (1.0 + 0x1p-20));
    *r_max = up(rmax * (1.0 + 0x1p-20));
    if (!std::isfinite(*radius)) *radius = 3.0e38f;
    if (!std::isfinite(*r_max)) *r_max = 3.0e38f;
}

MirtBvhPlan bvh_plan_of(const BvhBuild& b)
{
    MirtBvhPlan p{};
    p.n_nodes = (uint32_t)b.nodes.size();
    p.n_leaves = b.n_leaves;
    p.n_leaf_spheres = (uint32_t)b.ids.size() - b.n_always;
    p.n_always = b.n_always;
    p.max_depth = b.max_depth;
    p.max_leaf = b.max_leaf;
    p.device_bytes = 64ull * b.nodes.size() + 20ull * b.ids.size();
    return p;
}

int build_bvh(const MirtSphere* s, uint32_t n, BvhBuild* out)
{
    try {
        *out = BvhBuild{};
        std::vector<Item> items;
        items.reserve(n);
        // the always-tested list: boxes that are not finite, then the largest spheres above MIRT_BVH_BIG_RADII median radii
        const std::vector<uint32_t> always = bvh_always_list(s, n);
        std::vector<unsigned char> in_always(n, 0);
        for (uint32_t i : always) in_always[i] = 1;
        out->n_always = (uint32_t)always.size();
        out->recs.reserve(4ull * n);
        out->ids.reserve(n);
        auto put = [&](uint32_t i) {
            const MirtSphere& sp = s[i];
            out->recs.insert(out->recs.end(), { sp.center[0], sp.center[1], sp.center[2], sp.radius * sp.radius });   // the IEEE product of PreparedSphere.rr
            out->ids.push_back(i);
        };
        for (uint32_t i : always) put(i);

        // tree items: every sphere not on the list (a non-finite one beyond the list's capacity gets an infinite box: always visited)
        Box world; world.clear();
        for (uint32_t i = 0; i < n; ++i) {
            if (in_always[i]) continue;
            Item it;
            it.id = i;
            const double r = std::fabs((double)s[i].radius);
            bool finite = std::isfinite(r);
            for (int k = 0; k < 3; ++k) finite = finite && std::isfinite((double)s[i].center[k]);
            for (int k = 0; k < 3; ++k) {
                const double c = s[i].center[k];
                const double pad = 0x1p-20 * (std::fabs(c) + r);          // outward rounding with room to spare
                it.box.lo[k] = finite ? (double)down(c - r - pad) : -INFINITY;
                it.box.hi[k] = finite ? (double)up(c + r + pad) : INFINITY;
                it.c[k] = finite ? c : 0.0;
            }
            if (finite) world.grow(it.box);
            items.push_back(it);
        }
        // the sphere around the tree's boxes and the largest radius (nearest_hit_bvh's rounding bound)
        if (!items.empty() && world.lo[0] <= world.hi[0]) {
            double cen[3], rad = 0.0, rmax = 0.0;
            for (int k = 0; k < 3; ++k) cen[k] = (float)(0.5 * (world.lo[k] + world.hi[k]));
            for (const Item& it : items) {
                double d2 = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double e = std::max(std::fabs(it.box.lo[k] - cen[k]), std::fabs(it.box.hi[k] - cen[k]));
                    d2 += e * e;
                }
                rad = std::max(rad, std::sqrt(d2));
                rmax = std::max(rmax, std::fabs((double)s[it.id].radius));
            }
            for (int k = 0; k < 3; ++k) out->centre[k] = (float)cen[k];
            bvh_round_bounds(rad, rmax, &out->radius, &out->r_max);
        }

        // depth-first build: a node's index is given when it is created, the children's references and boxes are filled in the parent
        struct Task { uint32_t b, e, depth, parent, side; };
        std::vector<Task> todo;
        todo.push_back(Task{ 0u, (uint32_t)items.size(), 0u, 0xffffffffu, 0u });
        while (!todo.empty()) {
            const Task t = todo.back();
            todo.pop_back();
            const uint32_t m = t.e - t.b;
            Box bx; bx.clear();
            for (uint32_t i = t.b; i < t.e; ++i) bx.grow(items[i].box);
            uint32_t ref;
            if (m <= MIRT_BVH_MAX_LEAF) {
                ref = kBvhLeaf | (m << 24) | (uint32_t)out->ids.size();
                for (uint32_t i = t.b; i < t.e; ++i) put(items[i].id);
                if (m > 0) {
                    out->n_leaves += 1;
                    out->max_depth = std::max(out->max_depth, t.depth);
                    out->max_leaf = std::max(out->max_leaf, m);
                }
            } else {
                ref = (uint32_t)out->nodes.size();
                BvhNode nd;
                std::memset(&nd, 0, sizeof nd);
                out->nodes.push_back(nd);
                const uint32_t mid = split(items, t.b, t.e, t.depth);
                todo.push_back(Task{ mid, t.e, t.depth + 1, ref, 1u });
                todo.push_back(Task{ t.b, mid, t.depth + 1, ref, 0u });
            }
            if (t.parent == 0xffffffffu) { out->root = ref; continue; }
            BvhNode& p = out->nodes[t.parent];
            float* lo = t.side ? p.rmin : p.lmin;
            float* hi = t.side ? p.rmax : p.lmax;
            for (int k = 0; k < 3; ++k) { lo[k] = down(bx.lo[k]); hi[k] = up(bx.hi[k]); }
            (t.side ? p.right : p.left) = ref;
        }
        return MIRT_OK;
    } catch (const std::bad_alloc&) {
        *out = BvhBuild{};
        return set_error(MIRT_ERR_ALLOC, "out of host memory building the BVH of %u spheres", n);
    }
}

}  // namespace mirt

extern "C" int mirt_bvh_plan(const MirtSphere* spheres, uint32_t n_spheres, MirtBvhPlan* out)
{
    if (!out || (n_spheres && !spheres)) return mirt::set_error(MIRT_ERR_NULL_POINTER, "spheres/out is null");
    if (n_spheres > MIRT_SCENE_HBM_MAX_SPHERES)
        return mirt::set_error(MIRT_ERR_SCENE_TOO_LARGE, "%u spheres exceed MIRT_SCENE_HBM_MAX_SPHERES", n_spheres);
    mirt::BvhBuild b;
    const int rc = mirt::build_bvh(spheres, n_spheres, &b);
    if (rc != MIRT_OK) return rc;
    *out = mirt::bvh_plan_of(b);
    return MIRT_OK;
}
