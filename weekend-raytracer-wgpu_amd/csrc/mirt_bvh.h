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

}  // namespace mirt
