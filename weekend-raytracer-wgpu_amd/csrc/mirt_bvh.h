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
    std::vector<uint32_t> level_first;         // first inner node of every level (breadth-first numbering); the last entry = n_nodes
};

// Builds the tree of `spheres` (host copy: the always list only) from their prepared device copy `d_prepared` ([n] PreparedSphere,
// already uploaded) on `stream`, into *d_bvh (nodes | records | ids, grown when too small).  Synchronous: the tree is ready when it
// returns.  `always` = bvh_always_list(spheres, n), or the same list from census_spheres_device.  MIRT_OK, MIRT_ERR_ALLOC or MIRT_ERR_HIP.
int build_bvh_device(const std::vector<uint32_t>& always, uint32_t n, const void* d_prepared, void* hip_stream, BvhDeviceScratch* scratch,
                     unsigned char** d_bvh, size_t* cap_bvh, BvhDeviceResult* out);

// ---- in-place updates (mirt_bvh_device.hip): mirt_ctx_update_spheres* ----
// What a refit needs beyond the tables, prepared at the first update of a scene and dropped by every set_scene: the always-tested list
// (ids[0 .. n_always), sorted), the level schedule, and the layout of the builder scratch while updates run:
//   pos[n] (the inverse of ids) | order[n_nodes] (host-built trees: node indices sorted by depth) | reductions.
// The records of a host update are staged in a buffer of their own that grows with the largest `count` seen (none for device sources).
// A device-built tree's levels are the contiguous ranges of BvhDeviceResult.level_first; a host-built tree's are ranges of `order`.
struct BvhRefit {
    bool     ready = false;
    bool     ordered = false;                  // levels index `order` instead of the nodes themselves
    std::vector<uint32_t> level_first;
    uint32_t n_always = 0;
    uint32_t always[MIRT_BVH_MAX_ALWAYS] = {};
    size_t   off_pos = 0, off_order = 0, off_part = 0, off_partd = 0, off_red = 0, off_d2 = 0;
};

// The tables of the scene a refit works on (MirtContext's fields, by value).
struct BvhTables {
    unsigned char* d_bvh = nullptr;            // nodes | records | ids
    size_t         off_recs = 0, off_ids = 0;
    void*          d_prepared = nullptr;       // [n] PreparedSphere
    uint32_t       n = 0, n_nodes = 0, n_always = 0, root = kBvhLeaf;
};

// Prepares `st` for the tree in `t` (no write to the scene's tables).  `device_levels`: the builder's level_first of a device-built
// tree, nullptr for a host-built one (its child references are read back once).  MIRT_OK, MIRT_ERR_ALLOC or MIRT_ERR_HIP.
int refit_prepare(BvhRefit* st, const BvhTables& t, const std::vector<uint32_t>* device_levels, void* hip_stream, BvhDeviceScratch* scratch);

// Spheres [first, first + count) take centre and radius from `src` ([count] MirtSphere, host memory or -- src_on_device -- memory of
// this device); rr / inv_r / radius and the test records follow on the device, every child box of the tree is recomputed bottom-up and
// the traversal bounds are reduced again.  Synchronous.  `parts_ms`, when not null: scatter, refit, bounds between events.
int refit_bvh_device(const BvhRefit& st, const BvhTables& t, void* hip_stream, BvhDeviceScratch* scratch, BvhDeviceScratch* stage, uint32_t first,
                     uint32_t count, const void* src, bool src_on_device, float centre[3], float* radius, float* r_max, float parts_ms[3]);

// ---- a new sphere table from device memory (mirt_bvh_device.hip): mirt_ctx_set_spheres* ----
// What set_scene learns from a scene's spheres, learnt on the device from [n] MirtSphere in device memory (4-byte aligned) and the
// resident MirtMaterial table.
struct SpheresCensus {
    bool     bad_material_index = false;       // a material_idx >= n_mats
    uint32_t routines_seen = 0;                // bit min(materials[mi].id, 4) of every sphere whose index is in range
    bool     has_image_texture = false;        // such a sphere's material has a texture larger than 1x1
    std::vector<uint32_t> always;              // == bvh_always_list of the same spheres
    float    census_ms = 0.0f, always_ms = 0.0f;   // between events, when timed
};

// The census and the always-tested list; writes `scratch` only (whatever a refit kept there is gone).  Synchronous.
int census_spheres_device(const void* d_wire, uint32_t n, const void* d_mats, uint32_t n_mats, void* hip_stream, BvhDeviceScratch* scratch, bool timed,
                          SpheresCensus* out);

// d_prepared[i] = the PreparedSphere of wire record i (op = routine_queue[min(id, 4)] of its material; 4 without one).  Queued on the
// stream; waits for it only when `ms` (the kernel's time) is asked for.
int prepare_spheres_device(const void* d_wire, uint32_t n, const void* d_mats, uint32_t n_mats, const uint32_t routine_queue[5], void* d_prepared,
                           void* hip_stream, float* ms);

// ---- the schedule of a sorted ray batch (mirt_bvh_device.hip): MIRT_RAYS_SORT, MIRT_RADIANCE_SORT ----
// mirt_ray_sort_code of include/mirt.h for one 32-byte record (origin at byte 0, direction at byte 16).  Host only.
uint32_t ray_sort_code(const float centre[3], float radius, const void* ray32);

// Queues, on the stream, the codes of [n] 32-byte ray records in device memory (4-byte aligned) and their stable sort: afterwards
// scratch->d + *off_order holds [n] uint32, the caller's index of the ray in every slot, ascending (code, index).  No host
// synchronisation unless the scratch must grow: then the device is waited for first (launches in flight may read the old one).
// MIRT_OK, MIRT_ERR_ALLOC (nothing queued) or MIRT_ERR_HIP.
int ray_sort_order(const void* d_rays, uint32_t n, const float centre[3], float radius, void* hip_stream, BvhDeviceScratch* scratch, size_t* off_order);

}  // namespace mirt
