// mirt_bvh_device.hip — the device builder of MIRT_SCENE_HBM scenes (MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE), for gfx950.
//
// The image of an HBM scene does not depend on the tree's shape: every sphere is tested with test_sphere, every
// child box contains the outward-rounded boxes of the spheres below it, and bvh_centre / bvh_radius / bvh_rmax bound what they
// claim to bound.  This builder keeps those three properties, leaves of at most MIRT_BVH_MAX_LEAF spheres and a depth of at most
// MIRT_BVH_MAX_DEPTH (the traversal stack of nearest_hit_bvh drops a push beyond it: a deeper tree renders a wrong image), and builds
// a Morton-order tree instead of the host's binned SAH tree:
//   1. the always-tested list is the host rule's (bvh_always_list on the host, or the same list made on the device by
//      census_spheres_device at the end of this file); tree item t is the t-th sphere not on it;
//   2. keys: the centroid box of the tree items (device reduction), every centre quantised inside it in fp64 to 13 bits per axis
//      (cubic cells: the longest extent divides every axis), and key = morton << 24 | t -- unique, so the sorted order is a pure
//      function of the input;
//   3. rocprim::radix_sort_keys over the 63 key bits;
//   4. the hierarchy, top-down and one level at a time over the sorted order (a split launch and a numbering launch per level): a
//      node owning [b, e) with e - b <= 4 is a leaf whose records are the sorted order placed after the always list; else it splits
//      where the highest differing bit of its first and last code flips (binary search), or at the object median b + (m + 1) / 2 when
//      all its codes are equal or the split would break the host's depth rule (d + 1 + ceil(log2(ceil(m_child / 4))) <= 32 for both
//      children).  Inner nodes are numbered breadth-first by a scan over the level (wave shuffles, a block scan, and the sums of the
//      blocks before this one) -- no atomic counter, so the tree's bytes do not depend on scheduling;
//   5. boxes bottom-up, from the deepest level: per sphere the host formula in fp64, rounded outwards; unions are min / max;
//   6. the world box, the largest |radius| and the largest squared corner distance as device max-reductions in a fixed order; the
//      roundings of bvh_round_bounds on the host.
// Nothing here spins or waits on another block, and no value depends on the order in which blocks run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "mirt_bvh.h"
#include "mirt_kernels.h"

namespace mirt {
int set_error(int status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // mirt_api.hip
}

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kReduceBlocks = 512;            // partials of the two reductions
constexpr uint32_t kCodeBits = 13;                 // per axis: 39 code bits above the 24 index bits
constexpr uint32_t kIndexBits = 24;
constexpr uint32_t kNumRed = 13;                   // cmin[3] cmax[3] wmin[3] wmax[3] rmax

struct AlwaysList {
    uint32_t n;
    uint32_t idx[MIRT_BVH_MAX_ALWAYS];             // sorted
};

// tree item t -> its sphere: the t-th index that is not on the (sorted) always list
__device__ inline uint32_t item_sphere(uint32_t t, const AlwaysList& al)
{
    uint32_t id = t;
    for (uint32_t j = 0; j < al.n; ++j) if (al.idx[j] <= id) ++id;
    return id;
}

__device__ inline bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// nextafter(f, -inf) / nextafter(f, +inf) of a float that is not NaN
__device__ inline float below(float f)
{
    if (f == 0.0f) return __uint_as_float(0x80000001u);
    const uint32_t b = __float_as_uint(f);
    return __uint_as_float(f > 0.0f ? b - 1u : b + 1u);
}
__device__ inline float above(float f)
{
    if (f == 0.0f) return __uint_as_float(0x00000001u);
    const uint32_t b = __float_as_uint(f);
    return __uint_as_float(f > 0.0f ? b + 1u : b - 1u);
}
// mirt_bvh.cpp: down / up
__device__ inline float down(double v) { float f = (float)v; if ((double)f > v) f = below(f); return f; }
__device__ inline float up(double v)   { float f = (float)v; if ((double)f < v) f = above(f); return f; }

// The box and the binning centre of one tree item, by the host's formula (mirt_bvh.cpp: build_bvh): a sphere whose centre or radius
// is not finite gets an infinite box and centre 0.
__device__ inline bool item_box(const mirt::PreparedSphere& sp, float lo[3], float hi[3], float cen[3])
{
    const float cf[3] = { sp.cx, sp.cy, sp.cz };
    const float rf = __builtin_fabsf(sp.radius);
    const bool finite = finite_f(rf) && finite_f(cf[0]) && finite_f(cf[1]) && finite_f(cf[2]);
    const double r = (double)rf;
    for (int k = 0; k < 3; ++k) {
        const double c = (double)cf[k];
        const double pad = 0x1p-20 * (__builtin_fabs(c) + r);
        lo[k] = finite ? down(c - r - pad) : -INFINITY;
        hi[k] = finite ? up(c + r + pad) : INFINITY;
        cen[k] = finite ? cf[k] : 0.0f;
    }
    return finite;
}

__device__ inline float min_lt(float a, float b) { return b < a ? b : a; }
__device__ inline float max_lt(float a, float b) { return a < b ? b : a; }

// red[k], k < kNumRed: min for k < 3 and 6 <= k < 9, max otherwise
__device__ inline float red_op(uint32_t k, float a, float b) { return (k < 3u || (k >= 6u && k < 9u)) ? min_lt(a, b) : max_lt(a, b); }
__device__ inline float red_identity(uint32_t k) { return (k < 3u || (k >= 6u && k < 9u)) ? INFINITY : (k == 12u ? 0.0f : -INFINITY); }

__device__ inline void block_reduce_red(float v[kNumRed], float* out)
{
    __shared__ float sh[kNumRed][kBlock];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = 0; k < kNumRed; ++k) sh[k][tid] = v[k];
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s) for (uint32_t k = 0; k < kNumRed; ++k) sh[k][tid] = red_op(k, sh[k][tid], sh[k][tid + s]);
        __syncthreads();
    }
    if (tid < kNumRed) out[tid] = sh[tid][0];
}

// centroid box, world box (finite items), largest |radius| -> partials[gridDim.x][kNumRed]
__global__ __launch_bounds__(kBlock) void bvh_reduce_kernel(const mirt::PreparedSphere* sph, uint32_t m, AlwaysList al, float* partials)
{
    float v[kNumRed];
    for (uint32_t k = 0; k < kNumRed; ++k) v[k] = red_identity(k);
    for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < m; t += gridDim.x * kBlock) {
        const mirt::PreparedSphere sp = sph[item_sphere(t, al)];
        float lo[3], hi[3], c[3];
        const bool finite = item_box(sp, lo, hi, c);
        for (int k = 0; k < 3; ++k) {
            v[k] = min_lt(v[k], c[k]);
            v[3 + k] = max_lt(v[3 + k], c[k]);
            if (finite) { v[6 + k] = min_lt(v[6 + k], lo[k]); v[9 + k] = max_lt(v[9 + k], hi[k]); }
        }
        v[12] = max_lt(v[12], __builtin_fabsf(sp.radius));          // a NaN radius never wins, as in std::max(rmax, NaN)
    }
    block_reduce_red(v, partials + (size_t)blockIdx.x * kNumRed);
}

// one block: partials[n_part] -> red[kNumRed]
__global__ __launch_bounds__(kBlock) void bvh_reduce_final_kernel(const float* partials, uint32_t n_part, float* red)
{
    float v[kNumRed];
    for (uint32_t k = 0; k < kNumRed; ++k) v[k] = red_identity(k);
    for (uint32_t i = threadIdx.x; i < n_part; i += kBlock)
        for (uint32_t k = 0; k < kNumRed; ++k) v[k] = red_op(k, v[k], partials[(size_t)i * kNumRed + k]);
    block_reduce_red(v, red);
}

__device__ inline void block_reduce_max_d(double v, double* out)
{
    __shared__ double sh[kBlock];
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s && sh[tid] < sh[tid + s]) sh[tid] = sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = sh[0];
}

// the largest squared distance from the world box's centre to the farthest corner of an item's box (mirt_bvh.cpp: rad, before its
// square root -- the root is monotone, so the maximum commutes with it)
__global__ __launch_bounds__(kBlock) void bvh_corner_kernel(const mirt::PreparedSphere* sph, uint32_t m, AlwaysList al, const float* red, double* partials)
{
    double cen[3];
    for (int k = 0; k < 3; ++k) cen[k] = (double)(float)(0.5 * ((double)red[6 + k] + (double)red[9 + k]));
    double best = 0.0;
    for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < m; t += gridDim.x * kBlock) {
        float lo[3], hi[3], c[3];
        item_box(sph[item_sphere(t, al)], lo, hi, c);
        double d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double a = __builtin_fabs((double)lo[k] - cen[k]), b = __builtin_fabs((double)hi[k] - cen[k]);
            const double e = a < b ? b : a;
            d2 += e * e;
        }
        if (best < d2) best = d2;
    }
    block_reduce_max_d(best, partials + blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void bvh_corner_final_kernel(const double* partials, uint32_t n_part, double* out)
{
    double best = 0.0;
    for (uint32_t i = threadIdx.x; i < n_part; i += kBlock) if (best < partials[i]) best = partials[i];
    block_reduce_max_d(best, out);
}

// 13 bits -> every third bit
__device__ inline uint64_t spread3(uint32_t v)
{
    uint64_t x = v & 0x1fffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(kBlock) void bvh_keys_kernel(const mirt::PreparedSphere* sph, uint32_t m, AlwaysList al, const float* red, uint64_t* keys)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= m) return;
    float lo[3], hi[3], c[3];
    item_box(sph[item_sphere(t, al)], lo, hi, c);
    // Cubic cells: every axis is divided by the box's LONGEST extent.  Dividing each axis by its own extent would spend a third of
    // the code's bits on the noise of a flat world's thin axis (a field of spheres resting on a plane), and every third split would
    // cut the set into two halves that overlap completely.  An axis without extent gets cell 0 this way; a box without any
    // (or with a non-finite one) gives cell 0 everywhere -- never a division by it.
    double ext = 0.0;
    for (int k = 0; k < 3; ++k) { const double e = (double)red[3 + k] - (double)red[k]; if (ext < e) ext = e; }
    uint32_t cell[3] = { 0u, 0u, 0u };
    if (ext > 0.0 && ext < INFINITY) {
        for (int k = 0; k < 3; ++k) {
            const double q = ((double)c[k] - (double)red[k]) / ext * (double)(1u << kCodeBits);
            cell[k] = q >= (double)((1u << kCodeBits) - 1u) ? (1u << kCodeBits) - 1u : (q > 0.0 ? (uint32_t)q : 0u);
        }
    }
    const uint64_t code = (spread3(cell[0]) << 2) | (spread3(cell[1]) << 1) | spread3(cell[2]);
    keys[t] = (code << kIndexBits) | (uint64_t)t;
}

// the topology, one entry per inner node in breadth-first order
struct Topo {
    uint32_t* b;          // first item of the node's range in the sorted order
    uint32_t* e;          // one past its last
    uint32_t* left;       // child references (kBvhLeaf | count << 24 | first record, or an inner node's index); between the two
    uint32_t* right;      // launches of a level: left = the split position, right = the block-local rank of its first inner child
};

__global__ void bvh_root_kernel(Topo T, uint32_t m)
{
    T.b[0] = 0u;
    T.e[0] = m;
}

__device__ inline uint32_t ceil_log2(uint32_t v) { return v <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(v - 1u); }
__device__ inline uint32_t median_levels(uint32_t m) { return ceil_log2((m + MIRT_BVH_MAX_LEAF - 1u) / MIRT_BVH_MAX_LEAF); }

// Level launch 1 of 2: the split of every node [first, first + count) at `depth`, and the rank of its inner children inside the block
__global__ __launch_bounds__(kBlock) void bvh_split_kernel(Topo T, const uint64_t* keys, uint32_t first, uint32_t count, uint32_t depth, uint32_t* block_sums)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t cnt = 0u, mid = 0u;
    if (i < count) {
        const uint32_t b = T.b[first + i], e = T.e[first + i], m = e - b;
        const uint32_t median = b + (m + 1u) / 2u;
        const uint64_t c0 = keys[b] >> kIndexBits, c1 = keys[e - 1u] >> kIndexBits;
        mid = median;
        if (c0 != c1) {
            const uint32_t bit = 63u - (uint32_t)__builtin_clzll(c0 ^ c1);       // the codes share every bit above it: 0 at b, 1 at e - 1
            uint32_t lo = b, hi = e - 1u;
            while (hi - lo > 1u) {
                const uint32_t h = lo + (hi - lo) / 2u;
                if (((keys[h] >> kIndexBits) >> bit) & 1u) hi = h; else lo = h;
            }
            // the depth rule: both children must still fit below MIRT_BVH_MAX_DEPTH with median splits
            if (depth + 1u + median_levels(hi - b) <= MIRT_BVH_MAX_DEPTH && depth + 1u + median_levels(e - hi) <= MIRT_BVH_MAX_DEPTH) mid = hi;
        }
        cnt = (mid - b > MIRT_BVH_MAX_LEAF ? 1u : 0u) + (e - mid > MIRT_BVH_MAX_LEAF ? 1u : 0u);
    }
    // exclusive scan of cnt over the block: wave shuffles, then the waves' totals
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = cnt;
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t up_v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up_v;
    }
    __shared__ uint32_t wave_tot[kBlock / 64];
    if (lane == 63u) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t base = 0u, total = 0u;
    for (uint32_t w = 0; w < kBlock / 64; ++w) { if (w < wave) base += wave_tot[w]; total += wave_tot[w]; }
    if (i < count) {
        T.left[first + i] = mid;
        T.right[first + i] = base + incl - cnt;
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// Level launch 2 of 2: number the inner children breadth-first (next = index of the next level's first node) and write both references
// stats: [0] = inner nodes of the next level, [1] = largest leaf, [2] = a node index beyond the capacity (never, by construction)
__global__ __launch_bounds__(kBlock) void bvh_emit_kernel(Topo T, uint32_t first, uint32_t count, uint32_t next, uint32_t cap, uint32_t n_always,
                                                          const uint32_t* block_sums, uint32_t* stats)
{
    __shared__ uint32_t sh[kBlock];
    uint32_t part = 0u;
    for (uint32_t j = threadIdx.x; j < blockIdx.x; j += kBlock) part += block_sums[j];
    sh[threadIdx.x] = part;
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const uint32_t before = sh[0];
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) stats[0] = before + block_sums[blockIdx.x];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t g = first + i;
    const uint32_t b = T.b[g], e = T.e[g], mid = T.left[g];
    uint32_t idx = next + before + T.right[g];
    uint32_t ref[2];
    const uint32_t cb[2] = { b, mid }, ce[2] = { mid, e };
    for (int side = 0; side < 2; ++side) {
        const uint32_t m = ce[side] - cb[side];
        if (m > MIRT_BVH_MAX_LEAF) {
            if (idx < cap) { T.b[idx] = cb[side]; T.e[idx] = ce[side]; } else atomicMax(&stats[2], 1u);
            ref[side] = idx++;
        } else {
            ref[side] = mirt::kBvhLeaf | (m << 24) | (n_always + cb[side]);
            atomicMax(&stats[1], m);
        }
    }
    T.left[g] = ref[0];
    T.right[g] = ref[1];
}

// the box of a child: a leaf's spheres by the host formula, or the union of an inner node's two (finished) child boxes
__device__ inline void child_box(uint32_t ref, const mirt::BvhNode* nodes, const uint64_t* keys, const mirt::PreparedSphere* sph, const AlwaysList& al,
                                 uint32_t n_always, float lo[3], float hi[3])
{
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    if (ref & mirt::kBvhLeaf) {
        const uint32_t j0 = (ref & 0xffffffu) - n_always, cnt = (ref >> 24) & 0x7fu;
        for (uint32_t j = j0; j < j0 + cnt; ++j) {
            float l[3], h[3], c[3];
            item_box(sph[item_sphere((uint32_t)(keys[j] & ((1ull << kIndexBits) - 1ull)), al)], l, h, c);
            for (int k = 0; k < 3; ++k) { lo[k] = min_lt(lo[k], l[k]); hi[k] = max_lt(hi[k], h[k]); }
        }
    } else {
        const mirt::BvhNode& nd = nodes[ref];
        for (int k = 0; k < 3; ++k) { lo[k] = min_lt(nd.lmin[k], nd.rmin[k]); hi[k] = max_lt(nd.lmax[k], nd.rmax[k]); }
    }
}

__global__ __launch_bounds__(kBlock) void bvh_boxes_kernel(Topo T, mirt::BvhNode* nodes, const uint64_t* keys, const mirt::PreparedSphere* sph, AlwaysList al,
                                                           uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t g = first + i;
    mirt::BvhNode nd;
    nd.left = T.left[g];
    nd.right = T.right[g];
    nd.pad_[0] = nd.pad_[1] = 0u;
    child_box(nd.left, nodes, keys, sph, al, al.n, nd.lmin, nd.lmax);
    child_box(nd.right, nodes, keys, sph, al, al.n, nd.rmin, nd.rmax);
    nodes[g] = nd;
}

// records {centre, r * r} and original ids: the always list, then the sorted order
__global__ __launch_bounds__(kBlock) void bvh_records_kernel(const mirt::PreparedSphere* sph, uint32_t n, AlwaysList al, const uint64_t* keys, float4* recs, uint32_t* ids)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t id = j < al.n ? al.idx[j] : item_sphere((uint32_t)(keys[j - al.n] & ((1ull << kIndexBits) - 1ull)), al);
    const mirt::PreparedSphere sp = sph[id];
    recs[j] = make_float4(sp.cx, sp.cy, sp.cz, sp.rr);
    ids[j] = id;
}

size_t align256(size_t v) { return (v + 255u) & ~(size_t)255u; }

#define BVH_HIP_TRY(expr)                                                                                             \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess)                                                                                         \
            return mirt::set_error(MIRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int grow(unsigned char** ptr, size_t* cap, size_t need)
{
    if (need <= *cap && *ptr) return MIRT_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    if (hipMalloc(ptr, need ? need : 1) != hipSuccess) {
        (void)hipGetLastError();
        return mirt::set_error(MIRT_ERR_ALLOC, "hipMalloc(%zu bytes) failed", need);
    }
    *cap = need ? need : 1;
    return MIRT_OK;
}

uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

// mirt_bvh.cpp: the sphere around the tree's boxes and the largest radius -- only with a finite item in the tree (else all zero)
void finish_bounds(const float h_red[kNumRed], double h_d2, float centre[3], float* radius, float* r_max)
{
    for (int k = 0; k < 3; ++k) centre[k] = 0.0f;
    *radius = *r_max = 0.0f;
    if (h_red[6] <= h_red[9]) {
        for (int k = 0; k < 3; ++k) centre[k] = (float)(0.5 * ((double)h_red[6 + k] + (double)h_red[9 + k]));
        mirt::bvh_round_bounds(std::sqrt(h_d2), (double)h_red[12], radius, r_max);
    }
}

}  // namespace

int mirt::build_bvh_device(const std::vector<uint32_t>& always, uint32_t n, const void* d_prepared, void* hip_stream, BvhDeviceScratch* scratch,
                           unsigned char** d_bvh, size_t* cap_bvh, BvhDeviceResult* out)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const mirt::PreparedSphere* sph = static_cast<const mirt::PreparedSphere*>(d_prepared);
    AlwaysList al{};
    al.n = (uint32_t)always.size();
    for (uint32_t j = 0; j < al.n; ++j) al.idx[j] = always[j];
    const uint32_t m = n - al.n;                     // tree items
    BvhDeviceResult r = *out;                        // keeps always_ms
    r.plan = MirtBvhPlan{};
    r.plan.n_always = al.n;
    r.plan.n_leaf_spheres = m;
    r.root = kBvhLeaf | (m <= MIRT_BVH_MAX_LEAF ? m << 24 : 0u) | al.n;
    for (int k = 0; k < 3; ++k) r.centre[k] = 0.0f;
    r.radius = r.r_max = 0.0f;
    r.levels = 0;

    // scratch: keys (in, sorted) | topology | block sums | reduction partials and results | level statistics | the sort's storage
    const size_t cap_nodes = m ? m : 1u;
    size_t sort_bytes = 0;
    if (m) BVH_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)m, 0u, kIndexBits + 3u * kCodeBits, stream));
    size_t off = 0;
    const size_t o_keys_in = off;  off += align256(8ull * cap_nodes);
    const size_t o_keys = off;     off += align256(8ull * cap_nodes);
    size_t o_topo[4];
    for (int k = 0; k < 4; ++k) { o_topo[k] = off; off += align256(4ull * cap_nodes); }
    const size_t o_sums = off;     off += align256(4ull * (blocks_for((uint32_t)cap_nodes) + 1u));
    const size_t o_part = off;     off += align256(sizeof(float) * kNumRed * kReduceBlocks);
    const size_t o_partd = off;    off += align256(sizeof(double) * kReduceBlocks);
    const size_t o_red = off;      off += align256(sizeof(float) * 16u);
    const size_t o_d2 = off;       off += align256(sizeof(double));
    const size_t o_stats = off;    off += align256(sizeof(uint32_t) * 4u);
    const size_t o_sort = off;     off += align256(sort_bytes);
    int rc;
    if ((rc = grow(&scratch->d, &scratch->cap, off)) != MIRT_OK) return rc;
    unsigned char* S = scratch->d;
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(S + o_keys_in);
    uint64_t* keys = reinterpret_cast<uint64_t*>(S + o_keys);
    Topo T{ reinterpret_cast<uint32_t*>(S + o_topo[0]), reinterpret_cast<uint32_t*>(S + o_topo[1]), reinterpret_cast<uint32_t*>(S + o_topo[2]),
            reinterpret_cast<uint32_t*>(S + o_topo[3]) };
    uint32_t* block_sums = reinterpret_cast<uint32_t*>(S + o_sums);
    float* partials = reinterpret_cast<float*>(S + o_part);
    double* partials_d = reinterpret_cast<double*>(S + o_partd);
    float* red = reinterpret_cast<float*>(S + o_red);
    double* d2 = reinterpret_cast<double*>(S + o_d2);
    uint32_t* stats = reinterpret_cast<uint32_t*>(S + o_stats);

    const bool timed = std::getenv("MIRT_BVH_TIMING") != nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (timed) {
        BVH_HIP_TRY(hipEventCreate(&ev0));
        if (hipEventCreate(&ev1) != hipSuccess) { (void)hipEventDestroy(ev0); return mirt::set_error(MIRT_ERR_HIP, "hipEventCreate failed"); }
        (void)hipEventRecord(ev0, stream);
    }
    struct EventGuard { hipEvent_t a, b; ~EventGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } guard{ ev0, ev1 };

    std::vector<uint32_t>& level_first = r.level_first;   // first node of every level; the last entry = n_nodes
    level_first.clear();
    uint32_t n_nodes = 0, max_leaf = m <= MIRT_BVH_MAX_LEAF ? m : 0u;
    float h_red[kNumRed];
    double h_d2 = 0.0;
    if (m) {
        const uint32_t rb = blocks_for(m) < kReduceBlocks ? blocks_for(m) : kReduceBlocks;
        bvh_reduce_kernel<<<rb, kBlock, 0, stream>>>(sph, m, al, partials);
        bvh_reduce_final_kernel<<<1, kBlock, 0, stream>>>(partials, rb, red);
        bvh_corner_kernel<<<rb, kBlock, 0, stream>>>(sph, m, al, red, partials_d);
        bvh_corner_final_kernel<<<1, kBlock, 0, stream>>>(partials_d, rb, d2);
        bvh_keys_kernel<<<blocks_for(m), kBlock, 0, stream>>>(sph, m, al, red, keys_in);
        BVH_HIP_TRY(hipGetLastError());
        BVH_HIP_TRY(rocprim::radix_sort_keys(S + o_sort, sort_bytes, keys_in, keys, (size_t)m, 0u, kIndexBits + 3u * kCodeBits, stream));
        BVH_HIP_TRY(hipMemsetAsync(stats, 0, sizeof(uint32_t) * 4u, stream));
        if (m > MIRT_BVH_MAX_LEAF) {
            bvh_root_kernel<<<1, 1, 0, stream>>>(T, m);
            uint32_t first = 0, count = 1, depth = 0;
            level_first.push_back(0u);
            while (count) {
                if (depth >= MIRT_BVH_MAX_DEPTH) return mirt::set_error(MIRT_ERR_HIP, "device BVH build: an inner node at depth %u", depth);
                const uint32_t next = first + count;
                bvh_split_kernel<<<blocks_for(count), kBlock, 0, stream>>>(T, keys, first, count, depth, block_sums);
                bvh_emit_kernel<<<blocks_for(count), kBlock, 0, stream>>>(T, first, count, next, (uint32_t)cap_nodes, al.n, block_sums, stats);
                BVH_HIP_TRY(hipGetLastError());
                uint32_t h_stats[4];
                BVH_HIP_TRY(hipMemcpyAsync(h_stats, stats, sizeof h_stats, hipMemcpyDeviceToHost, stream));
                BVH_HIP_TRY(hipStreamSynchronize(stream));
                if (h_stats[2] || (uint64_t)next + h_stats[0] > cap_nodes)
                    return mirt::set_error(MIRT_ERR_HIP, "device BVH build: more inner nodes than spheres (%u + %u of %u)", next, h_stats[0], m);
                max_leaf = h_stats[1];
                level_first.push_back(next);
                first = next;
                count = h_stats[0];
                ++depth;
            }
            n_nodes = first;
            r.levels = depth;                          // levels of inner nodes; the deepest leaves hang one below the last
            r.root = 0u;
        }
        BVH_HIP_TRY(hipMemcpyAsync(h_red, red, sizeof h_red, hipMemcpyDeviceToHost, stream));
        BVH_HIP_TRY(hipMemcpyAsync(&h_d2, d2, sizeof h_d2, hipMemcpyDeviceToHost, stream));
    }

    // the tables: nodes | records | ids, each 16-byte aligned (64 n_nodes and 16 n are)
    const size_t nb = (size_t)n_nodes * sizeof(BvhNode), rbytes = (size_t)n * 16u, ib = (size_t)n * 4u;
    if ((rc = grow(d_bvh, cap_bvh, nb + rbytes + ib + 16u)) != MIRT_OK) return rc;
    r.off_recs = nb;
    r.off_ids = nb + rbytes;
    BvhNode* nodes = reinterpret_cast<BvhNode*>(*d_bvh);
    if (n) bvh_records_kernel<<<blocks_for(n), kBlock, 0, stream>>>(sph, n, al, keys, reinterpret_cast<float4*>(*d_bvh + r.off_recs),
                                                                    reinterpret_cast<uint32_t*>(*d_bvh + r.off_ids));
    for (size_t l = level_first.size(); l-- > 1;) {                      // boxes, from the deepest level up
        const uint32_t first = level_first[l - 1], count = level_first[l] - first;
        bvh_boxes_kernel<<<blocks_for(count), kBlock, 0, stream>>>(T, nodes, keys, sph, al, first, count);
    }
    BVH_HIP_TRY(hipGetLastError());
    if (timed) (void)hipEventRecord(ev1, stream);
    BVH_HIP_TRY(hipStreamSynchronize(stream));
    if (timed) { float ms = 0.0f; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) r.kernels_ms = ms; }

    r.plan.n_nodes = n_nodes;
    r.plan.n_leaves = n_nodes ? n_nodes + 1u : (m ? 1u : 0u);          // every inner node has two children, every leaf at least one sphere
    r.plan.max_depth = n_nodes ? r.levels : 0u;
    r.plan.max_leaf = max_leaf;
    r.plan.device_bytes = 64ull * n_nodes + 20ull * n;
    // mirt_bvh.cpp: the sphere around the tree's boxes and the largest radius -- only with a finite item in the tree
    if (m) finish_bounds(h_red, h_d2, r.centre, &r.radius, &r.r_max);
    *out = r;
    return MIRT_OK;
}

// ---- in-place updates: mirt_ctx_update_spheres*  ----
// The exactness argument never uses the tree's shape, so moved spheres keep the topology, the ids table and the always-tested list of
// the scene as it was set: 1. scatter the new centres and radii into the prepared spheres and the test records, 2. recompute every
// child box bottom-up, one launch per level (no atomics, nothing waits on another block), 3. reduce the traversal bounds again in the
// builder's fixed order.  Works on a tree of either builder.
namespace {

// pos[ids[j]] = j: the record of every sphere
__global__ __launch_bounds__(kBlock) void bvh_pos_kernel(const uint32_t* ids, uint32_t n, uint32_t* pos)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n) pos[ids[j]] = j;
}

// src: [count] MirtSphere (8 words: centre[4], radius, material_idx, 2 x pad); only the centre and the radius are read.
// r * r and 1.0f / r are the single IEEE operations of set_scene (this file is compiled without contraction, with the correctly
// rounded division).
__global__ __launch_bounds__(kBlock) void bvh_scatter_kernel(const float* src, uint32_t first, uint32_t count, const uint32_t* pos,
                                                             mirt::PreparedSphere* sph, float4* recs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const float* in = src + 8ull * i;
    const float cx = in[0], cy = in[1], cz = in[2], r = in[4];
    const float rr = r * r;
    const uint32_t id = first + i;
    mirt::PreparedSphere& o = sph[id];
    o.cx = cx; o.cy = cy; o.cz = cz; o.rr = rr;
    o.inv_r = 1.0f / r;
    o.radius = r;
    recs[pos[id]] = make_float4(cx, cy, cz, rr);
}

// child_box with the spheres of a leaf taken from the ids table (ref's low bits index the records, always list included)
__device__ inline void refit_child_box(uint32_t ref, const mirt::BvhNode* nodes, const uint32_t* ids, const mirt::PreparedSphere* sph, float lo[3], float hi[3])
{
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    if (ref & mirt::kBvhLeaf) {
        const uint32_t j0 = ref & 0xffffffu, cnt = (ref >> 24) & 0x7fu;
        for (uint32_t j = j0; j < j0 + cnt; ++j) {
            float l[3], h[3], c[3];
            item_box(sph[ids[j]], l, h, c);
            for (int k = 0; k < 3; ++k) { lo[k] = min_lt(lo[k], l[k]); hi[k] = max_lt(hi[k], h[k]); }
        }
    } else {
        const mirt::BvhNode& nd = nodes[ref];
        for (int k = 0; k < 3; ++k) { lo[k] = min_lt(nd.lmin[k], nd.rmin[k]); hi[k] = max_lt(nd.lmax[k], nd.rmax[k]); }
    }
}

// one level: node order[first + i] (order == nullptr: node first + i); its children's boxes are finished (deeper levels ran before)
__global__ __launch_bounds__(kBlock) void bvh_refit_kernel(mirt::BvhNode* nodes, const uint32_t* order, uint32_t first, uint32_t count, const uint32_t* ids,
                                                           const mirt::PreparedSphere* sph)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t g = order ? order[first + i] : first + i;
    mirt::BvhNode nd = nodes[g];
    refit_child_box(nd.left, nodes, ids, sph, nd.lmin, nd.lmax);
    refit_child_box(nd.right, nodes, ids, sph, nd.rmin, nd.rmax);
    nodes[g] = nd;
}

}  // namespace

int mirt::refit_prepare(BvhRefit* st, const BvhTables& t, const std::vector<uint32_t>* device_levels, void* hip_stream, BvhDeviceScratch* scratch)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    BvhRefit s;
    s.n_always = t.n_always;
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(t.d_bvh + t.off_ids);
    if (t.n_always > MIRT_BVH_MAX_ALWAYS || t.n_always > t.n) return mirt::set_error(MIRT_ERR_HIP, "refit: an always-tested list of %u", t.n_always);
    if (t.n_always) BVH_HIP_TRY(hipMemcpy(s.always, ids, 4ull * t.n_always, hipMemcpyDeviceToHost));
    std::sort(s.always, s.always + s.n_always);
    std::vector<uint32_t> order;
    try {
        if (device_levels) {
            s.level_first = *device_levels;
        } else if (t.n_nodes) {
            // a host-built tree: {left, right} of every node, once; breadth-first from the root gives the nodes sorted by depth
            std::vector<uint32_t> kids(2ull * t.n_nodes);
            BVH_HIP_TRY(hipMemcpy2D(kids.data(), 8, t.d_bvh + offsetof(BvhNode, left), sizeof(BvhNode), 8, t.n_nodes, hipMemcpyDeviceToHost));
            order.reserve(t.n_nodes);
            if ((t.root & kBvhLeaf) || t.root >= t.n_nodes) return mirt::set_error(MIRT_ERR_HIP, "refit: root %#x of a tree of %u nodes", t.root, t.n_nodes);
            order.push_back(t.root);
            s.level_first.push_back(0u);
            size_t level_begin = 0;
            while (level_begin < order.size()) {
                const size_t level_end = order.size();
                for (size_t q = level_begin; q < level_end; ++q)
                    for (int side = 0; side < 2; ++side) {
                        const uint32_t ref = kids[2ull * order[q] + side];
                        if (ref & kBvhLeaf) continue;
                        if (ref >= t.n_nodes || order.size() >= t.n_nodes)
                            return mirt::set_error(MIRT_ERR_HIP, "refit: child reference %u of node %u in a tree of %u nodes", ref, order[q], t.n_nodes);
                        order.push_back(ref);
                    }
                level_begin = level_end;
                s.level_first.push_back((uint32_t)level_end);
            }
            s.ordered = true;
        }
    } catch (const std::bad_alloc&) {
        return mirt::set_error(MIRT_ERR_ALLOC, "out of host memory preparing the refit of %u nodes", t.n_nodes);
    }
    const size_t cap_n = t.n ? t.n : 1u;
    size_t off = 0;
    s.off_pos = off;    off += align256(4ull * cap_n);
    s.off_order = off;  off += align256(4ull * (order.size() ? order.size() : 1u));
    s.off_part = off;   off += align256(sizeof(float) * kNumRed * kReduceBlocks);
    s.off_partd = off;  off += align256(sizeof(double) * kReduceBlocks);
    s.off_red = off;    off += align256(sizeof(float) * 16u);
    s.off_d2 = off;     off += align256(sizeof(double));
    int rc;
    if ((rc = grow(&scratch->d, &scratch->cap, off)) != MIRT_OK) return rc;
    if (!order.empty()) BVH_HIP_TRY(hipMemcpy(scratch->d + s.off_order, order.data(), 4ull * order.size(), hipMemcpyHostToDevice));
    if (t.n) {
        bvh_pos_kernel<<<blocks_for(t.n), kBlock, 0, stream>>>(ids, t.n, reinterpret_cast<uint32_t*>(scratch->d + s.off_pos));
        BVH_HIP_TRY(hipGetLastError());
        BVH_HIP_TRY(hipStreamSynchronize(stream));
    }
    s.ready = true;
    *st = std::move(s);
    return MIRT_OK;
}

int mirt::refit_bvh_device(const BvhRefit& st, const BvhTables& t, void* hip_stream, BvhDeviceScratch* scratch, BvhDeviceScratch* stage, uint32_t first,
                           uint32_t count, const void* src, bool src_on_device, float centre[3], float* radius, float* r_max, float parts_ms[3])
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned char* S = scratch->d;
    mirt::PreparedSphere* sph = static_cast<mirt::PreparedSphere*>(t.d_prepared);
    BvhNode* nodes = reinterpret_cast<BvhNode*>(t.d_bvh);
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(t.d_bvh + t.off_ids);
    const uint32_t* order = st.ordered ? reinterpret_cast<const uint32_t*>(S + st.off_order) : nullptr;
    float* partials = reinterpret_cast<float*>(S + st.off_part);
    double* partials_d = reinterpret_cast<double*>(S + st.off_partd);
    float* red = reinterpret_cast<float*>(S + st.off_red);
    double* d2 = reinterpret_cast<double*>(S + st.off_d2);
    AlwaysList al{};
    al.n = st.n_always;
    for (uint32_t j = 0; j < al.n; ++j) al.idx[j] = st.always[j];
    const uint32_t m = t.n - al.n;

    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    struct EventGuard { hipEvent_t* e; ~EventGuard() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ ev };
    if (parts_ms) for (int k = 0; k < 4; ++k) BVH_HIP_TRY(hipEventCreate(&ev[k]));

    const float* d_src = static_cast<const float*>(src);
    if (!src_on_device) {                                  // staged in a buffer that grows with the largest host update
        int rc;
        if ((rc = grow(&stage->d, &stage->cap, 32ull * count)) != MIRT_OK) return rc;
        BVH_HIP_TRY(hipMemcpy(stage->d, src, 32ull * count, hipMemcpyHostToDevice));
        d_src = reinterpret_cast<const float*>(stage->d);
    }
    if (parts_ms) (void)hipEventRecord(ev[0], stream);
    bvh_scatter_kernel<<<blocks_for(count), kBlock, 0, stream>>>(d_src, first, count, reinterpret_cast<const uint32_t*>(S + st.off_pos), sph,
                                                                 reinterpret_cast<float4*>(t.d_bvh + t.off_recs));
    if (parts_ms) (void)hipEventRecord(ev[1], stream);
    for (size_t l = st.level_first.size(); l-- > 1;) {     // boxes, from the deepest level up
        const uint32_t lf = st.level_first[l - 1], cnt = st.level_first[l] - lf;
        if (cnt) bvh_refit_kernel<<<blocks_for(cnt), kBlock, 0, stream>>>(nodes, order, lf, cnt, ids, sph);
    }
    if (parts_ms) (void)hipEventRecord(ev[2], stream);
    float h_red[kNumRed];
    double h_d2 = 0.0;
    if (m) {
        const uint32_t rb = blocks_for(m) < kReduceBlocks ? blocks_for(m) : kReduceBlocks;
        bvh_reduce_kernel<<<rb, kBlock, 0, stream>>>(sph, m, al, partials);
        bvh_reduce_final_kernel<<<1, kBlock, 0, stream>>>(partials, rb, red);
        bvh_corner_kernel<<<rb, kBlock, 0, stream>>>(sph, m, al, red, partials_d);
        bvh_corner_final_kernel<<<1, kBlock, 0, stream>>>(partials_d, rb, d2);
        BVH_HIP_TRY(hipGetLastError());
        BVH_HIP_TRY(hipMemcpyAsync(h_red, red, sizeof h_red, hipMemcpyDeviceToHost, stream));
        BVH_HIP_TRY(hipMemcpyAsync(&h_d2, d2, sizeof h_d2, hipMemcpyDeviceToHost, stream));
    }
    BVH_HIP_TRY(hipGetLastError());
    if (parts_ms) (void)hipEventRecord(ev[3], stream);
    BVH_HIP_TRY(hipStreamSynchronize(stream));
    if (parts_ms) for (int k = 0; k < 3; ++k) { parts_ms[k] = 0.0f; (void)hipEventElapsedTime(&parts_ms[k], ev[k], ev[k + 1]); }
    for (int k = 0; k < 3; ++k) centre[k] = 0.0f;
    *radius = *r_max = 0.0f;
    if (m) finish_bounds(h_red, h_d2, centre, radius, r_max);
    return MIRT_OK;
}

// ---- a new sphere table from wire records in device memory: mirt_ctx_set_spheres*  ----
// Everything set_scene derives from the spheres on the host, derived on the device from [n] MirtSphere (8 words: centre[4], radius,
// material_idx, 2 x pad; words 3, 6 and 7 are never read; 4-byte aligned) and the resident MirtMaterial table: the census (is a
// material index out of range, which scatter routines occur, does a used material carry an image texture), the always-tested list
// of bvh_always_list, and the PreparedSphere table.  As above, nothing waits on another block and every result is a pure function of
// the input.
namespace {

constexpr uint32_t kCensusBadIndex = 1u << 5;      // above the five routine bits
constexpr uint32_t kCensusImage = 1u << 6;
constexpr uint32_t kAlwaysKeyBits = 57;            // 24 index bits, 32 radius bits, the "box is not finite" bit
constexpr uint64_t kAlwaysBad = 1ull << 56;

__device__ inline void block_reduce_or(uint32_t v, uint32_t* out)
{
    __shared__ uint32_t sh[kBlock];
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] |= sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) *out = sh[0];
}

// routines seen (bit min(id, 4) of every sphere with a material) | kCensusBadIndex | kCensusImage -> partials[gridDim.x]
__global__ __launch_bounds__(kBlock) void census_kernel(const uint32_t* wire, uint32_t n, const MirtMaterial* mats, uint32_t n_mats, uint32_t* partials)
{
    uint32_t v = 0u;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t mi = wire[8ull * i + 5u];
        if (mi >= n_mats) { v |= kCensusBadIndex; continue; }
        const MirtMaterial m = mats[mi];
        v |= 1u << (m.id < 4u ? m.id : 4u);
        if ((uint64_t)m.desc1.width * m.desc1.height > 1u || (uint64_t)m.desc2.width * m.desc2.height > 1u) v |= kCensusImage;
    }
    block_reduce_or(v, partials + blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void census_final_kernel(const uint32_t* partials, uint32_t n_part, uint32_t* out)
{
    uint32_t v = 0u;
    for (uint32_t i = threadIdx.x; i < n_part; i += kBlock) v |= partials[i];
    block_reduce_or(v, out);
}

// One key per sphere whose ascending order is: the spheres with a finite box by |radius| descending, ties by index ascending, then
// the others by index.  bvh_always_list's test of a box (mirt_bvh.cpp), in fp64: c - r and c + r of two finite floats are finite.
__global__ __launch_bounds__(kBlock) void always_keys_kernel(const float* wire, uint32_t n, uint64_t* keys)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* in = wire + 8ull * i;
    const float r = __builtin_fabsf(in[4]);
    bool ok = finite_f(r);
    for (int k = 0; k < 3; ++k) {
        const float c = in[k];
        ok = ok && finite_f(c) && __builtin_fabs((double)c) + (double)r < 3.0e38;
    }
    keys[i] = ok ? ((uint64_t)(0xffffffffu - __float_as_uint(r)) << kIndexBits) | (uint64_t)i : kAlwaysBad | (uint64_t)i;
}

// One block of MIRT_BVH_MAX_ALWAYS threads over the sorted keys: the first spheres without a finite box, then -- while room is left --
// the largest of those above MIRT_BVH_BIG_RADII median radii; the list sorted by index (every thread ranks its own entry).
__global__ __launch_bounds__(MIRT_BVH_MAX_ALWAYS) void always_list_kernel(const uint64_t* keys, uint32_t n, AlwaysList* out)
{
    __shared__ uint32_t sh_idx[MIRT_BVH_MAX_ALWAYS];
    __shared__ uint32_t sh_valid[MIRT_BVH_MAX_ALWAYS];
    // m = the spheres with a finite box = the first key with kAlwaysBad (every thread searches: 24 reads of the same words)
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t h = lo + (hi - lo) / 2u;
        if (keys[h] < kAlwaysBad) lo = h + 1u; else hi = h;
    }
    const uint32_t m = lo, n_bad = n - m, nb = n_bad < MIRT_BVH_MAX_ALWAYS ? n_bad : MIRT_BVH_MAX_ALWAYS;
    const uint32_t j = threadIdx.x;
    uint32_t idx = 0u, valid = 0u;
    if (j < nb) {
        idx = (uint32_t)(keys[m + j] & ((1ull << kIndexBits) - 1ull));
        valid = 1u;
    } else if (j - nb < m) {
        // the median: position m / 2 of the ascending radii = position m - 1 - m / 2 here
        const float median = __uint_as_float(0xffffffffu - (uint32_t)(keys[m - 1u - m / 2u] >> kIndexBits));
        const uint64_t key = keys[j - nb];
        const float r = __uint_as_float(0xffffffffu - (uint32_t)(key >> kIndexBits));
        idx = (uint32_t)(key & ((1ull << kIndexBits) - 1ull));
        valid = (double)r > (double)MIRT_BVH_BIG_RADII * (double)median ? 1u : 0u;
    }
    sh_idx[j] = idx;
    sh_valid[j] = valid;
    __syncthreads();
    uint32_t rank = 0u, total = 0u;
    for (uint32_t k = 0; k < MIRT_BVH_MAX_ALWAYS; ++k) {
        total += sh_valid[k];
        if (sh_valid[k] && sh_idx[k] < idx) ++rank;
    }
    if (valid) out->idx[rank] = idx;
    if (j == 0) out->n = total;
}

struct QueueMap { uint32_t q[5]; };               // routine min(id, 4) -> queue of the pool kernel

// wire record -> PreparedSphere; r * r and 1.0f / r are the single IEEE operations of set_scene
__global__ __launch_bounds__(kBlock) void prepare_kernel(const float* wire, uint32_t n, const MirtMaterial* mats, uint32_t n_mats, QueueMap map,
                                                         mirt::PreparedSphere* sph)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* in = wire + 8ull * i;
    const float r = in[4];
    const uint32_t mi = reinterpret_cast<const uint32_t*>(in)[5];
    uint32_t routine = 4u;
    if (mi < n_mats) { const uint32_t id = mats[mi].id; if (id < 4u) routine = id; }
    mirt::PreparedSphere o;
    o.cx = in[0]; o.cy = in[1]; o.cz = in[2];
    o.rr = r * r;
    o.inv_r = 1.0f / r;
    o.radius = r;
    o.material_idx = mi;
    o.op = map.q[routine];
    sph[i] = o;
}

struct Events {
    hipEvent_t e[4] = { nullptr, nullptr, nullptr, nullptr };
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

int mirt::census_spheres_device(const void* d_wire, uint32_t n, const void* d_mats, uint32_t n_mats, void* hip_stream, BvhDeviceScratch* scratch,
                                bool timed, SpheresCensus* out)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    SpheresCensus r;
    if (!n) { *out = std::move(r); return MIRT_OK; }
    // scratch: keys (in, sorted) | census partials | census word | the list | the sort's storage
    size_t sort_bytes = 0;
    BVH_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0u, kAlwaysKeyBits, stream));
    size_t off = 0;
    const size_t o_keys_in = off;  off += align256(8ull * n);
    const size_t o_keys = off;     off += align256(8ull * n);
    const size_t o_part = off;     off += align256(sizeof(uint32_t) * kReduceBlocks);
    const size_t o_word = off;     off += align256(sizeof(uint32_t));
    const size_t o_list = off;     off += align256(sizeof(AlwaysList));
    const size_t o_sort = off;     off += align256(sort_bytes);
    int rc;
    if ((rc = grow(&scratch->d, &scratch->cap, off)) != MIRT_OK) return rc;
    unsigned char* S = scratch->d;
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(S + o_keys_in);
    uint64_t* keys = reinterpret_cast<uint64_t*>(S + o_keys);
    uint32_t* partials = reinterpret_cast<uint32_t*>(S + o_part);
    uint32_t* word = reinterpret_cast<uint32_t*>(S + o_word);
    AlwaysList* list = reinterpret_cast<AlwaysList*>(S + o_list);

    Events ev;
    if (timed) for (int k = 0; k < 3; ++k) BVH_HIP_TRY(hipEventCreate(&ev.e[k]));
    if (timed) (void)hipEventRecord(ev.e[0], stream);
    const uint32_t rb = blocks_for(n) < kReduceBlocks ? blocks_for(n) : kReduceBlocks;
    census_kernel<<<rb, kBlock, 0, stream>>>(static_cast<const uint32_t*>(d_wire), n, static_cast<const MirtMaterial*>(d_mats), n_mats, partials);
    census_final_kernel<<<1, kBlock, 0, stream>>>(partials, rb, word);
    if (timed) (void)hipEventRecord(ev.e[1], stream);
    always_keys_kernel<<<blocks_for(n), kBlock, 0, stream>>>(static_cast<const float*>(d_wire), n, keys_in);
    BVH_HIP_TRY(hipGetLastError());
    BVH_HIP_TRY(rocprim::radix_sort_keys(S + o_sort, sort_bytes, keys_in, keys, (size_t)n, 0u, kAlwaysKeyBits, stream));
    always_list_kernel<<<1, MIRT_BVH_MAX_ALWAYS, 0, stream>>>(keys, n, list);
    BVH_HIP_TRY(hipGetLastError());
    if (timed) (void)hipEventRecord(ev.e[2], stream);
    uint32_t h_word = 0;
    AlwaysList h_list{};
    BVH_HIP_TRY(hipMemcpyAsync(&h_word, word, sizeof h_word, hipMemcpyDeviceToHost, stream));
    BVH_HIP_TRY(hipMemcpyAsync(&h_list, list, sizeof h_list, hipMemcpyDeviceToHost, stream));
    BVH_HIP_TRY(hipStreamSynchronize(stream));
    if (timed) {
        (void)hipEventElapsedTime(&r.census_ms, ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&r.always_ms, ev.e[1], ev.e[2]);
    }
    if (h_list.n > MIRT_BVH_MAX_ALWAYS || h_list.n > n) return mirt::set_error(MIRT_ERR_HIP, "set_spheres: an always-tested list of %u", h_list.n);
    r.routines_seen = h_word & 31u;
    r.bad_material_index = (h_word & kCensusBadIndex) != 0u;
    r.has_image_texture = (h_word & kCensusImage) != 0u;
    try {
        r.always.assign(h_list.idx, h_list.idx + h_list.n);
    } catch (const std::bad_alloc&) {
        return mirt::set_error(MIRT_ERR_ALLOC, "out of host memory");
    }
    *out = std::move(r);
    return MIRT_OK;
}

int mirt::prepare_spheres_device(const void* d_wire, uint32_t n, const void* d_mats, uint32_t n_mats, const uint32_t routine_queue[5], void* d_prepared,
                                 void* hip_stream, float* ms)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (ms) *ms = 0.0f;
    if (!n) return MIRT_OK;
    QueueMap map;
    for (int k = 0; k < 5; ++k) map.q[k] = routine_queue[k];
    Events ev;
    if (ms) for (int k = 0; k < 2; ++k) BVH_HIP_TRY(hipEventCreate(&ev.e[k]));
    if (ms) (void)hipEventRecord(ev.e[0], stream);
    prepare_kernel<<<blocks_for(n), kBlock, 0, stream>>>(static_cast<const float*>(d_wire), n, static_cast<const MirtMaterial*>(d_mats), n_mats, map,
                                                         static_cast<mirt::PreparedSphere*>(d_prepared));
    BVH_HIP_TRY(hipGetLastError());
    if (ms) {                                              // untimed: the builder that follows on this stream waits for it
        (void)hipEventRecord(ev.e[1], stream);
        BVH_HIP_TRY(hipStreamSynchronize(stream));
        (void)hipEventElapsedTime(ms, ev.e[0], ev.e[1]);
    }
    return MIRT_OK;
}

// ---- the schedule of a sorted ray batch (MIRT_RAYS_SORT, MIRT_RADIANCE_SORT; include/mirt.h) ----
namespace {

typedef uint32_t trace_u4 __attribute__((ext_vector_type(4), aligned(4)));      // mirt_trace_kernel.inc: a caller's records are 4-byte aligned

// q(f, n) of the header: 0 for anything that is not above 0 (NaN included), n - 1 from n on, truncation between
__host__ __device__ inline uint32_t sort_q(float f, uint32_t n)
{
    if (!(f > 0.0f)) return 0u;
    if (f >= (float)n) return n - 1u;
    return (uint32_t)f;
}

// The 31-bit code of the header, one IEEE operation per line of its text (this file is compiled with -ffp-contract=off and correctly
// rounded division on both sides, so the host and the device agree bit for bit).  lo[k] = centre[k] - radius, inv = 16.0f / radius.
__host__ __device__ inline uint32_t ray_code(const float o[3], const float d[3], const float lo[3], float inv)
{
    uint32_t c[3];
    for (int k = 0; k < 3; ++k) c[k] = sort_q((o[k] - lo[k]) * inv, 1u << MIRT_RAY_SORT_ORIGIN_BITS);
    const float s = (__builtin_fabsf(d[0]) + __builtin_fabsf(d[1])) + __builtin_fabsf(d[2]);
    const float r = 1.0f / s;
    float u = d[0] * r, v = d[1] * r;
    if (d[2] < 0.0f) {
        const float fu = (1.0f - __builtin_fabsf(v)) * (u >= 0.0f ? 1.0f : -1.0f);
        const float fv = (1.0f - __builtin_fabsf(u)) * (v >= 0.0f ? 1.0f : -1.0f);
        u = fu;
        v = fv;
    }
    const float half = (float)(1u << (MIRT_RAY_SORT_DIRECTION_BITS - 1u));
    const uint32_t a = sort_q(u * half + half, 1u << MIRT_RAY_SORT_DIRECTION_BITS);
    const uint32_t b = sort_q(v * half + half, 1u << MIRT_RAY_SORT_DIRECTION_BITS);
    uint32_t m3 = 0u, m2 = 0u;
    for (uint32_t j = 0; j < MIRT_RAY_SORT_ORIGIN_BITS; ++j)
        m3 |= (((c[0] >> j) & 1u) << (3u * j + 2u)) | (((c[1] >> j) & 1u) << (3u * j + 1u)) | (((c[2] >> j) & 1u) << (3u * j));
    for (uint32_t j = 0; j < MIRT_RAY_SORT_DIRECTION_BITS; ++j)
        m2 |= (((a >> j) & 1u) << (2u * j + 1u)) | (((b >> j) & 1u) << (2u * j));
    return (m3 << (2u * MIRT_RAY_SORT_DIRECTION_BITS)) | m2;
}
static_assert(3u * MIRT_RAY_SORT_ORIGIN_BITS + 2u * MIRT_RAY_SORT_DIRECTION_BITS == 31u, "the sort runs over 31 key bits");

struct SortBounds { float lo[3]; float inv; };

// lane = ray: two 16-byte loads, the code and the ray's own index out
__global__ __launch_bounds__(kBlock) void ray_codes_kernel(const trace_u4* rays, uint32_t n_rays, SortBounds B, uint32_t* codes, uint32_t* index)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_rays) return;
    const trace_u4 r0 = rays[2u * i], r1 = rays[2u * i + 1u];          // {origin, t_max | stream} {direction, _pad}
    const float o[3] = { __uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z) };
    const float d[3] = { __uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z) };
    codes[i] = ray_code(o, d, B.lo, B.inv);
    index[i] = (uint32_t)i;
}

SortBounds sort_bounds(const float centre[3], float radius)
{
    SortBounds b;
    for (int k = 0; k < 3; ++k) b.lo[k] = centre[k] - radius;
    b.inv = 16.0f / radius;
    return b;
}

}  // namespace

uint32_t mirt::ray_sort_code(const float centre[3], float radius, const void* ray32)
{
    float f[8];
    std::memcpy(f, ray32, sizeof f);
    const SortBounds b = sort_bounds(centre, radius);
    return ray_code(f, f + 4, b.lo, b.inv);
}

int mirt::ray_sort_order(const void* d_rays, uint32_t n, const float centre[3], float radius, void* hip_stream, BvhDeviceScratch* scratch, size_t* off_order)
{
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    constexpr unsigned kKeyBits = 3u * MIRT_RAY_SORT_ORIGIN_BITS + 2u * MIRT_RAY_SORT_DIRECTION_BITS;
    size_t sort_bytes = 0;
    BVH_HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u,
                                          kKeyBits, stream));
    // scratch: the order | codes (in, sorted) | indices in | the sort's storage
    size_t off = 0;
    const size_t o_order = off;    off += align256(4ull * n);
    const size_t o_codes_in = off; off += align256(4ull * n);
    const size_t o_codes = off;    off += align256(4ull * n);
    const size_t o_index = off;    off += align256(4ull * n);
    const size_t o_sort = off;     off += align256(sort_bytes);
    if (off > scratch->cap || !scratch->d) {
        BVH_HIP_TRY(hipDeviceSynchronize());      // sorted launches may still read the old scratch, on any stream
        int rc;
        if ((rc = grow(&scratch->d, &scratch->cap, off)) != MIRT_OK) return rc;
    }
    unsigned char* S = scratch->d;
    uint32_t* codes_in = reinterpret_cast<uint32_t*>(S + o_codes_in);
    uint32_t* index = reinterpret_cast<uint32_t*>(S + o_index);
    ray_codes_kernel<<<(uint32_t)(((uint64_t)n + kBlock - 1u) / kBlock), kBlock, 0, stream>>>(static_cast<const trace_u4*>(d_rays), n, sort_bounds(centre, radius), codes_in, index);
    BVH_HIP_TRY(hipGetLastError());
    // stable: equal codes keep the caller's order
    BVH_HIP_TRY(rocprim::radix_sort_pairs(S + o_sort, sort_bytes, codes_in, reinterpret_cast<uint32_t*>(S + o_codes), index, reinterpret_cast<uint32_t*>(S + o_order),
                                          (size_t)n, 0u, kKeyBits, stream));
    *off_order = o_order;
    return MIRT_OK;
}
