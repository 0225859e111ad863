// mirt_bvh.h — the host BVH builder of MIRT_SCENE_HBM scenes (mirt_bvh.cpp) and the device tables it produces.
// Plain host C++: compiled into libmirt.so by g++, included by mirt_api.hip.
#pragma once

#include <stdint.h>
#include <vector>

#include "../../include/mirt.h"

namespace mirt {

// One inner node, 64 bytes: the boxes of BOTH children (so a visit reads one line and tests two boxes) and the two child references.
// A reference with kBvhLeaf set is a leaf: bits 24..30 = sphere count (0 .. MIRT_BVH_MAX_LEAF; 0 = nothing to test), bits 0..23 = its
// first test record.  Otherwise it is an inner node's index.
struct BvhNode {
    float    lmin[3], lmax[3];
    float    rmin[3], rmax[3];
    uint32_t left, right;
    uint32_t pad_[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode is one 64-byte line");
constexpr uint32_t kBvhLeaf = 0x80000000u;

struct BvhBuild {
    std::vector<BvhNode>  nodes;
    std::vector<float>    recs;        // [n_spheres][4] = {centre, r * r}: the always-tested list first, then the leaves' spheres in leaf order
    std::vector<uint32_t> ids;         // [n_spheres]: the original sphere index of every record
    uint32_t root = kBvhLeaf;          // reference of the root (an empty tree: a leaf of 0 spheres)
    uint32_t n_always = 0, n_leaves = 0, max_depth = 0, max_leaf = 0;
    // what the traversal's rounding bound needs (mirt_kernels.hip: nearest_hit_bvh): a sphere around every tree sphere's box, and the
    // largest |radius| in the tree -- both rounded up
    float    centre[3] = {0.0f, 0.0f, 0.0f};
    float    radius = 0.0f;
    float    r_max = 0.0f;
};

// Builds the tree over spheres[0 .. n) (n <= MIRT_SCENE_HBM_MAX_SPHERES).  Deterministic.  MIRT_OK or MIRT_ERR_ALLOC.
int build_bvh(const MirtSphere* spheres, uint32_t n, BvhBuild* out);

// The always-tested list of those spheres, sorted by index (at most MIRT_BVH_MAX_ALWAYS entries): the spheres whose box is not finite,
// in index order, then the largest of those above MIRT_BVH_BIG_RADII median radii (ties to the lower index).  One rule for both
// builders (build_bvh above, build_bvh_device below).  O(n); may throw std::bad_alloc.
std::vector<uint32_t> bvh_always_list(const MirtSphere* spheres, uint32_t n);

// bvh_radius / bvh_rmax from the exact maxima `rad` (distance from the centre to the farthest box corner) and `rmax` (largest
// |radius|): rounded up with a 2^-20 margin, clamped to 3.0e38.
void bvh_round_bounds(double rad, double rmax, float* radius, float* r_max);

// MirtBvhPlan of a finished host build
MirtBvhPlan bvh_plan_of(const BvhBuild& b);

// ---- the device builder (mirt_bvh_device.hip): MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE ----
// Scratch of the device builder (sort keys, the level-by-level topology, reduction partials, the sort's temporary storage): owned by
// the context, grows, never shrinks.
struct BvhDeviceScratch {
    unsigned char* d = nullptr;
    size_t         cap = 0;
};

struct BvhDeviceResult {
    MirtBvhPlan plan{};
    uint32_t    root = kBvhLeaf;
    float       centre[3] = {0.0f, 0.0f, 0.0f};
    float       radius = 0.0f, r_max = 0.0f;
    size_t      off_recs = 0, off_ids = 0;     // byte offsets of the records / ids in *d_bvh (nodes at 0)
    double      always_ms = 0.0;               // host: the always-tested list
    double      kernels_ms = 0.0;              // device: first launch to the tree being ready
    uint32_t    levels = 0;
};

// Builds the tree of `spheres` (host copy: the always list only) from their prepared device copy `d_prepared` ([n] PreparedSphere,
// already uploaded) on `stream`, into *d_bvh (nodes | records | ids, grown when too small).  Synchronous: the tree is ready when it
// returns.  `always` = bvh_always_list(spheres, n).  MIRT_OK, MIRT_ERR_ALLOC or MIRT_ERR_HIP.
int build_bvh_device(const std::vector<uint32_t>& always, uint32_t n, const void* d_prepared, void* hip_stream, BvhDeviceScratch* scratch,
                     unsigned char** d_bvh, size_t* cap_bvh, BvhDeviceResult* out);

}  // namespace mirt
