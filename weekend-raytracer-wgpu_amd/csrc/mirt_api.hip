// mirt_api.hip — the C ABI of include/mirt.h: host-side validation, scene residency, kernel
// launches and timing.  No CPU rendering path exists here: without a HIP device every render
// entry point fails with MIRT_ERR_NO_DEVICE.
//
// Host arithmetic that the reference also does on the host (GpuCamera::new, camera_orientation,
// Angle, RenderParams::validate) is restated here in f32 without contraction
// (-ffp-contract=off applies to host code too).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/mirt.h"
#include "mirt_kernels.h"
#include "mirt_bvh.h"
#include "mirt_adapt_rule.h"

namespace kx = mirt::exact_build;     // the kernels of the bit-exact build (default)
namespace kf = mirt::fast_build;      // MIRT_FLAG_FAST_MATH: the same kernels with hardware transcendentals

namespace {

thread_local char g_err[512] = "";

int fail(int status, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return status;
}

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(MIRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

using mirt::rows_valid;     // MirtParams row selection, the knobs and the pooled BVH geometry: mirt_launch_plan.h
using mirt::out_rows;
using mirt::Tuning;
using mirt::plan_bvh_pool;

bool desc_ok(const MirtTextureDescriptor& d, uint64_t n_texels)
{
    if (d.width == 0 || d.height == 0) return false;
    return (uint64_t)d.offset + (uint64_t)d.width * (uint64_t)d.height <= n_texels;
}

// jenkinsHash (raytracer.wgsl:513-521) — used to fold the 64-bit seed into the stream key
uint32_t jenkins_hash(uint32_t x)
{
    x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15;
    return x;
}

constexpr int kEventPool = 64;
constexpr int kDispenserStride = MIRT_DISPENSER_STRIDE;             // u32 words between the eight dispenser words of a launch (mirt_kernels.h)
constexpr int kDispenserWords = 8 * kDispenserStride;

constexpr float kRustPi = 3.14159265358979323846f;   // std::f32::consts::PI

struct V3 { float x, y, z; };
// nalgebra 3-vector arithmetic (no fusion): dot = (a0*b0 + a1*b1) + a2*b2; normalize = v / sqrt(dot)
float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
V3 normalize3(V3 a) { const float n = std::sqrt(dot3(a, a)); return V3{ a.x / n, a.y / n, a.z / n }; }
V3 cross3(V3 a, V3 b) { return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
V3 scale3(float s, V3 a) { return V3{ s * a.x, s * a.y, s * a.z }; }
V3 add3(V3 a, V3 b) { return V3{ a.x + b.x, a.y + b.y, a.z + b.z }; }
V3 sub3(V3 a, V3 b) { return V3{ a.x - b.x, a.y - b.y, a.z - b.z }; }

// Build the uniform grid of mirt_kernels.h over the spheres of a many-sphere scene.  Returns an empty
// blob when a grid would not help (few spheres, or nothing small enough to bin) -- or when THIS cell size lists more
// than 65 535 items (`*overflow` = true: a coarser cell may still work, mirt_ctx_set_scene retries).
std::vector<unsigned char> build_grid(const MirtSphere* sph, uint32_t n, double cell_factor_knob, double big_factor_knob, bool* overflow = nullptr)
{
    std::vector<unsigned char> blob;
    if (overflow) *overflow = false;
    if (n < mirt::kGridMinSpheres || n > 65535u) return blob;
    std::vector<float> radii(n);
    for (uint32_t i = 0; i < n; ++i) radii[i] = std::fabs(sph[i].radius);
    std::vector<float> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const float r_med = sorted[n / 2];
    if (!(r_med > 0.0f) || !std::isfinite(r_med)) return blob;
    // spheres up to `big_factor` median radii go into the grid; the rest (ground planes) are tested for every ray
    const float big_factor = (float)(big_factor_knob > 0.0 ? big_factor_knob : 4.0);
    std::vector<uint16_t> big, small;
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (uint32_t i = 0; i < n; ++i) {
        const bool finite = std::isfinite(sph[i].center[0]) && std::isfinite(sph[i].center[1]) && std::isfinite(sph[i].center[2]) && std::isfinite(radii[i]);
        if (!finite || radii[i] > big_factor * r_med) { big.push_back((uint16_t)i); continue; }
        small.push_back((uint16_t)i);
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], (double)sph[i].center[k] - radii[i]);
            hi[k] = std::max(hi[k], (double)sph[i].center[k] + radii[i]);
        }
    }
    if (small.size() < mirt::kGridMinSpheres / 2 || big.size() > 64) return blob;
    // cell = 2.5 median radii (a binned sphere of up to 4 median radii spans at most 5 cells per axis).  Measured on RTIOW, 1080p x 128 spp,
    // records stored once per sphere: 4 -> 14.31 ms, 3.5 -> 13.95, 3 -> 13.35, 2.75 -> 13.38, 2.5 -> 13.18, 2.25 -> 13.11, 2 -> 19.7 (the cell
    // table outgrows LDS: 128-slot pools); fewer tests per ray against more cells per ray (profiles/r03_c5_ab.txt blocks 4 and 7)
    const double cell_factor = cell_factor_knob > 0.0 ? cell_factor_knob : 2.5;   // mirt_ctx_set_scene passes the factor it settles on
    double cell = cell_factor * r_med;
    // What the enlargement `eps` of the binning must absorb (the argument is written out above GridLds in mirt_kernels.hip):
    //   e_disc  the rounding of the SPHERE TEST: the flat scan reports a hit at a point up to sqrt(r^2 + K u L^2) from the centre of a
    //           sphere (c, r), L = |o - c| + |r|, K u = 35 * 2^-24.  sqrt(r^2 + x) - r falls as r grows, so the smallest binned |r|
    //           bounds it for every binned sphere, for every ray with L <= L_safe.  L_safe = kGridSafeReach x R_g covers the scene's
    //           own extent and an eye next to it (R_g: radius of a sphere around all binned spheres); rays from farther away are
    //           recognised by their origin and do not rely on the binning (GridHeader.guard).  e_disc is held to a quarter cell --
    //           tiny spheres in coarse cells -- by shrinking L_safe instead.
    //   e_walk  the rounding of the WALK: cell faces fma(i, cell, org) and entry points are rounded at the size M of the scene's
    //           coordinates (2 u M each), a crossing parameter carries a few u, and `tx += ddx` adds one u per step, all relative to
    //           a parameter whose point lies within L of the origin: 2^-22 M + 2^-23 (steps + 16) L_safe, plus the 1e-3 cell of old.
    // The grid's box is grown by eps as well, so a reported hit point always lies INSIDE the box the walk is clipped to.
    constexpr double kDiscErr = 35.0 * 0x1p-24, kGridSafeReach = 2.5;
    double r_min = 1e300, cg[3], rg2 = 0.0, coord_max = 0.0;
    for (uint16_t i : small) r_min = std::min(r_min, (double)radii[i]);
    for (int k = 0; k < 3; ++k) {
        cg[k] = 0.5 * (lo[k] + hi[k]);
        rg2 += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]);
        coord_max = std::max(coord_max, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
    }
    const double rg = std::sqrt(rg2);
    uint32_t dims[3];
    double eps = 0.0, l_safe = 0.0, glo[3], ghi[3];
    for (;;) {
        l_safe = kGridSafeReach * rg;
        double e_disc = std::sqrt(r_min * r_min + kDiscErr * l_safe * l_safe) - r_min;
        if (e_disc > 0.25 * cell) {
            e_disc = 0.25 * cell;
            l_safe = std::sqrt(((r_min + e_disc) * (r_min + e_disc) - r_min * r_min) / kDiscErr);
        }
        // The dims are counted in double and converted only once they are known to be small: a world whose extent is 2^32 cells or
        // more (spheres of radius 2^-29 along 80 octaves) made the conversion itself undefined -- dims of 0, a grid of no cells that
        // "fits", and a write into its first list.
        double ddims[3] = { 16.0, 16.0, 16.0 }, total = 1.0;
        for (int pass = 0; pass < 2; ++pass) {                    // the step count of e_walk comes from the dims: settle them in two passes
            const double steps = ddims[0] + ddims[1] + ddims[2];
            eps = 1e-3 * cell + 0x1p-22 * coord_max + 0x1p-23 * (steps + 16.0) * l_safe + e_disc;
            total = 1.0;
            for (int k = 0; k < 3; ++k) {
                glo[k] = lo[k] - eps; ghi[k] = hi[k] + eps;
                ddims[k] = std::max(1.0, std::ceil((ghi[k] - glo[k]) / cell + 1e-6)); total *= ddims[k];
            }
        }
        if (total <= (double)mirt::kGridMaxCells) {
            for (int k = 0; k < 3; ++k) dims[k] = (uint32_t)ddims[k];
            break;
        }
        cell *= 1.26;
    }
    for (int k = 0; k < 3; ++k) lo[k] = glo[k];                   // the grid's lower corner: the spheres' box grown by eps
    const uint32_t ncells = dims[0] * dims[1] * dims[2];
    std::vector<std::vector<uint16_t>> lists(ncells);
    for (uint16_t i : small) {
        int c0[3], c1[3];
        for (int k = 0; k < 3; ++k) {
            c0[k] = (int)std::floor(((double)sph[i].center[k] - radii[i] - eps - lo[k]) / cell);
            c1[k] = (int)std::floor(((double)sph[i].center[k] + radii[i] + eps - lo[k]) / cell);
            c0[k] = std::max(0, std::min((int)dims[k] - 1, c0[k]));
            c1[k] = std::max(0, std::min((int)dims[k] - 1, c1[k]));
        }
        for (int z = c0[2]; z <= c1[2]; ++z)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int x = c0[0]; x <= c1[0]; ++x) lists[((size_t)z * dims[1] + y) * dims[0] + x].push_back(i);   // ascending ids
    }
    size_t n_items = 0, n_entries = 0;
    for (auto& l : lists) {
        n_entries += l.size();
        n_items += l.size() > 2 ? l.size() - 2 : 0;             // the first two ids of a cell live in its table entry
    }
    if (n_entries > 65535u) { if (overflow) *overflow = true; return blob; }     // cell_start is 16 bit
    mirt::GridHeader h{};
    for (int k = 0; k < 3; ++k) {
        h.org[k] = (float)lo[k];
        h.cell[k] = (float)cell;
        h.inv_cell[k] = (float)(1.0 / cell);
        h.dims[k] = dims[k];
    }
    h.n_big = (uint32_t)big.size();
    const size_t hdr_u16 = sizeof(mirt::GridHeader) / 2;
    h.off_big = (uint32_t)hdr_u16;
    h.off_items = h.off_big + (uint32_t)big.size();
    size_t bytes = ((size_t)h.off_items + n_items) * 2;
    h.off_ops = (uint32_t)bytes;                                  // u8 per sphere, filled by the caller (needs the materials)
    bytes = (bytes + n + 7) & ~size_t(7);
    h.off_cells = (uint32_t)bytes;                                // two u32 per cell: first further item | count << 16, id0 | id1 << 16
    bytes = (bytes + 8 * (size_t)ncells + 15) & ~size_t(15);
    h.n_entries = (uint32_t)n_entries;
    h.n_spheres = n;
    const double far_d = l_safe / 1.02 - rg;                      // 2 %: the kernels' float arithmetic on |o - C_g|^2, R_g rounded below
    for (int k = 0; k < 3; ++k) h.guard[k] = (float)cg[k];
    h.guard[3] = far_d > 0.0 ? (float)(far_d * far_d) : -1.0f;
    h.bound_r = (float)(rg * 1.0001);
    h.inv_dim_x = 1.0f / (float)dims[0];
    h.inv_dim_xy = 1.0f / (float)(dims[0] * dims[1]);
    h.off_big_recs = (uint32_t)bytes;
    bytes += big.size() * 16;
    h.off_recs = (uint32_t)bytes;
    bytes += (size_t)n * 16;                                      // one record per SPHERE, indexed by sphere id
    h.total_bytes = (uint32_t)bytes;
    blob.assign(h.total_bytes, 0);
    uint16_t* u = reinterpret_cast<uint16_t*>(blob.data());
    uint32_t* cells = reinterpret_cast<uint32_t*>(blob.data() + h.off_cells);
    std::memcpy(blob.data(), &h, sizeof h);
    // test record of sphere i: centre and r*r, the first half of its PreparedSphere (same IEEE product as set_scene's)
    auto put_rec = [&](size_t byte_off, uint16_t i) {
        const float rec[4] = { sph[i].center[0], sph[i].center[1], sph[i].center[2], sph[i].radius * sph[i].radius };
        std::memcpy(blob.data() + byte_off, rec, 16);
    };
    for (size_t i = 0; i < big.size(); ++i) { u[h.off_big + i] = big[i]; put_rec(h.off_big_recs + 16 * i, big[i]); }
    uint32_t pos = 0;
    for (uint32_t c = 0; c < ncells; ++c) {
        const auto& l = lists[c];
        cells[2 * c] = pos | ((uint32_t)l.size() << 16);
        cells[2 * c + 1] = (l.size() > 0 ? (uint32_t)l[0] : 0u) | ((l.size() > 1 ? (uint32_t)l[1] : 0u) << 16);   // absent: sphere 0 (valid, never tested)
        for (size_t k = 2; k < l.size(); ++k) u[h.off_items + pos++] = l[k];
    }
    for (uint32_t i = 0; i < n; ++i) put_rec(h.off_recs + 16 * (size_t)i, (uint16_t)i);
    return blob;
}

// The grid mirt_ctx_set_scene keeps: the default cell of 2.5 median radii, coarsened (x 1.26 per step, up to the 4 median radii of
// round 2 and no further) while the blob would not leave the pooled kernel the 152-slot geometry RTIOW runs (kGridPoolSlotChoices:
// 160 only fits beside smaller blobs and measured no better) -- or while the cell is so fine that the lists overflow their 16-bit
// index (bimodal radii: a sphere of 4 median radii spans 5 cells per axis at 2.5, 3 at 4): such a scene built a grid at round 2's
// cell of 4 and must not lose it to the finer default.  `cell_knob` > 0 (MIRT_GRID_CELL) forces one cell size.
std::vector<unsigned char> plan_grid(const MirtSphere* sph, uint32_t n, double cell_knob, double big_knob, size_t lds_per_block, double* factor_out)
{
    std::vector<unsigned char> grid;
    double f = cell_knob > 0.0 ? cell_knob : 2.5;
    for (;; f = std::min(f * 1.26, 4.0)) {
        bool overflow = false;
        grid = build_grid(sph, n, f, big_knob, &overflow);
        if (cell_knob > 0.0 || f >= 4.0) break;                                // a forced cell, or the coarsest one: take what it gives
        if (grid.empty()) { if (overflow) continue; break; }                   // too many entries: coarser; a grid would not help: none
        const size_t beside = kx::scene_lds_bytes_grid(n, true) + grid.size();
        if (beside < lds_per_block && kx::pool_config_grid(lds_per_block - beside, false).slots >= 152u) break;
    }
    if (factor_out) *factor_out = grid.empty() ? 0.0 : f;
    return grid;
}

// The knobs of mirt_launch_plan.h's Tuning, read from the environment (once per context: mirt_ctx_create).
Tuning read_tuning()
{
    Tuning t;
    if (const char* e = std::getenv("MIRT_POOL_CONFIG")) { const long v = std::strtol(e, nullptr, 10); if (v >= 0 && (uint32_t)v < kx::pool_config_count()) t.pool_config = (int)v; }
    if (const char* e = std::getenv("MIRT_POOL_GRID")) t.pool_grid = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_STRIP_MODE")) t.fixed_strips = e[0] == '1';
    if (const char* e = std::getenv("MIRT_GSS_MINW")) { const uint32_t v = (uint32_t)std::atoi(e); if (v >= 1 && v <= 16) t.gss_min_width = v; }
    if (const char* e = std::getenv("MIRT_GSS_KEEP")) { const double v = std::atof(e); if (v > 0.0 && v < 64.0) t.gss_keep = v; }
    if (const char* e = std::getenv("MIRT_BY_PIXEL")) t.by_pixel = (e[0] == '1') ? 1 : 0;
    if (const char* e = std::getenv("MIRT_POOL_BLOCKS_PER_CU")) { const uint32_t v = (uint32_t)std::atoi(e); if (v >= 1) t.pool_blocks_per_cu = v; }
    if (const char* e = std::getenv("MIRT_GRID_CELL")) { const double v = std::atof(e); if (v >= 1.0 && v <= 64.0) t.grid_cell = v; }
    if (const char* e = std::getenv("MIRT_PINHOLE")) t.pinhole = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_SPREAD_UNITS")) t.spread_units = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_STATIC_UNITS")) t.static_units = (e[0] == '1') ? 1 : 0;
    if (const char* e = std::getenv("MIRT_POOL_MIN_SPP")) { const int v = std::atoi(e); if (v >= 1) t.pool_min_spp = v; }
    if (const char* e = std::getenv("MIRT_STREAM")) t.stream = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = std::getenv("MIRT_PX_GROUPS")) { const int v = std::atoi(e); if (v >= 0 && v <= 3) t.px_groups = v; }
    if (const char* e = std::getenv("MIRT_STRIP_CAND")) t.strip_cand = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_GRID_FLAT_Y")) t.grid_flat_y = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_DEBUG_SLOTS")) t.debug_slots = e[0] == '1';
    if (const char* e = std::getenv("MIRT_STATIC_BLOCK")) { const int v = std::atoi(e); if (v == 64 || v == 128 || v == 256) t.static_block = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_STATIC_GRID")) { const int v = std::atoi(e); if (v >= 1 && v <= 64) t.static_grid = v; }
    if (const char* e = std::getenv("MIRT_TIMING")) t.timing = (e[0] == '0') ? 0 : 1;
    if (const char* e = std::getenv("MIRT_EXT_EVENTS")) t.ext_events = e[0] != '0';
    if (const char* e = std::getenv("MIRT_HBM_POOL_SLOTS")) {
        const uint32_t v = (uint32_t)std::atoi(e);
        for (uint32_t s : mirt::kBvhPoolSlotChoices) if (v == s) t.hbm_pool_slots = v;
    }
    if (const char* e = std::getenv("MIRT_RADIANCE_POOL_BLOCKS")) { const int v = std::atoi(e); if (v >= 1) t.radiance_pool_blocks = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_ADAPT_POOL_BLOCKS")) { const int v = std::atoi(e); if (v >= 1) t.adapt_pool_blocks = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_ADAPT_LDS_BLOCKS")) { const int v = std::atoi(e); if (v >= 1) t.adapt_lds_blocks = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_QUERY_LDS_BLOCKS")) { const int v = std::atoi(e); if (v >= 1) t.query_lds_blocks = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_DENOISE_STAGED")) { const int v = std::atoi(e); if (v >= 0 && v <= 255) t.denoise_staged = v; }
    if (const char* e = std::getenv("MIRT_ADAPT_LDS_GROUPS")) { const int v = std::atoi(e); if (v >= 1 && v <= 3) t.adapt_lds_groups = (uint32_t)v; }
    if (const char* e = std::getenv("MIRT_GRID_BIG")) { const double v = std::atof(e); if (v >= 1.0 && v <= 1024.0) t.grid_big = v; }
    return t;
}

// A camera whose thin-lens offset is exactly zero for every lens draw, so that `origin = eye + lens_radius * (...)`
// (wgsl:468-472) is `eye` bit for bit: lens_radius == +-0 (aperture 0: GpuCamera::new mod.rs:705), a finite lens basis and a
// finite eye without a -0 component (see generate_primary in mirt_kernels.hip for the argument).
bool camera_is_pinhole(const MirtGpuCamera& cam)
{
    if (cam.lens_radius != 0.0f) return false;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(cam.u[k]) || !std::isfinite(cam.v[k]) || !std::isfinite(cam.eye[k])) return false;
        if (cam.eye[k] == 0.0f && std::signbit(cam.eye[k])) return false;
    }
    return true;
}

template <typename T>
int ensure_capacity(T** ptr, size_t* cap, size_t need)
{
    if (need <= *cap && *ptr) return MIRT_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    const size_t bytes = (need ? need : 1) * sizeof(T);
    if (hipMalloc(ptr, bytes) != hipSuccess) return fail(MIRT_ERR_ALLOC, "hipMalloc(%zu bytes) failed", bytes);
    *cap = need ? need : 1;
    return MIRT_OK;
}

}  // namespace

// the message of a failing C-ABI call, for the library's other translation units (mirt_node.hip)
int mirt::set_error(int status, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return status;
}

struct MirtContext {
    int         device = -1;
    int         cu_count = 0;
    size_t      lds_per_block = 65536, lds_per_cu = 65536;
    hipStream_t stream = nullptr;
    // hipEvent pairs around every render kernel, recorded on the stream the kernel runs on;
    // drained (summed) by mirt_ctx_get_stats so that no host sync sits inside a timed loop.
    // The slots form a RING: a launch takes the next slot; the slots half a ring ahead are retired in batches of 16 (launches 17 to 32
    // launches old, normally long finished: waits that return at once) -- no drain of the whole pool, nothing that stalls a caller who
    // queues launches back to back (the reference's interactive loop: one set_data / render_frame per displayed frame).
    std::vector<hipEvent_t> ev_begin, ev_end;
    std::vector<hipEvent_t> ev_zeroed;            // per slot: its dispenser words are zero again (recorded on zero_stream)
    std::vector<unsigned char> slot_busy;         // a launch is recorded in the slot and not yet folded into ms_folded
    std::vector<unsigned char> slot_dirty;        // the slot's launch took units from its dispenser words: they must be re-zeroed before the next use
    std::vector<unsigned char> slot_zeroing;      // a re-zeroing of the slot's dispenser words is queued (ev_zeroed says when it is done)
    std::vector<unsigned char> slot_zero_event;   // ... and which ev_zeroed: the slot's own, or its batch's first slot (retire_slots)
    std::vector<unsigned char> slot_timed;        // the slot's launch carries a start AND an end event (kernel time is folded into the statistics)
    bool        timing = true;                    // mirt_ctx_set_timing: launches carry an event pair (mirt_ctx_get_stats reports kernel times)
    std::vector<hipStream_t> untimed_streams;     // caller streams that carried launches without an end event (mirt_ctx_synchronize covers them)
    size_t      ev_next = 0;          // slot of the next launch
    size_t      ev_in_flight = 0;     // busy slots: the ring positions ev_next - ev_in_flight .. ev_next - 1
    hipStream_t zero_stream = nullptr;            // re-zeroes the dispenser words of retired slots, off the callers' streams
    hipStream_t frame_stream_b = nullptr;         // mirt_ctx_frame_stream(ctx, 1): a second stream on another hardware queue (created on first use)
    double      ms_folded = 0.0;      // time of the launches already retired
    uint64_t    launches_folded = 0;
    double      last_ms = 0.0;

    // resident scene
    bool     have_scene = false;
    uint32_t n_spheres = 0, n_mats = 0;
    uint64_t n_texels = 0;
    bool     have_sky = false;
    float    sph3[12] = {};               // {centre, r^2} of the spheres of a three-sphere scene (RenderArgs.sph3)
    bool     has_image_texture = false;   // a material refers to a texture larger than 1x1
    uint32_t n_shading_routines = 0;      // distinct scatter routines the spheres' materials select
    uint32_t queue_routine[5] = {0, 1, 2, 3, 4};   // dense numbering of the routines present (pool kernel queues)
    int      pt_scene_status = MIRT_OK;
    int      parity_scene_status = MIRT_OK;
    // the materials' part of the two verdicts, kept for mirt_ctx_set_spheres*: what the tables say whatever the spheres are
    int      pt_materials_status = MIRT_OK;
    int      parity_materials_status = MIRT_OK;   // of a world that is not empty
    MirtGpuCamera         cam{};          // host copy; travels by value with every launch (RenderArgs.cam)
    mirt::PreparedSphere* d_spheres = nullptr;
    MirtMaterial*         d_mats = nullptr;
    mirt::PreparedMaterial* d_pmats = nullptr;
    size_t cap_pmats = 0;
    unsigned char* d_grid = nullptr;        // uniform grid blob (many-sphere scenes), see build_grid
    size_t cap_grid = 0;
    mirt::ShadeRec* d_shade = nullptr;      // [n_spheres] shading records of the grid builds (sphere + its material in one line)
    size_t cap_shade = 0;
    uint32_t grid_bytes = 0;
    bool     have_shade = false;             // d_shade holds this scene's records
    bool     grid_packable = false;          // the grid has at most kGridMaxCells cells: a parked walk's linear cell index fits 16 bits (always, as built)
    bool     grid_flat_y = false;            // the grid is ONE cell high (dims[1] == 1: spheres on a ground plane): the pooled kernel walks it in two dimensions
    bool     fits_flat = true;               // spheres + materials fit the LDS budget (flat kernels usable)
    float*                d_texels = nullptr;
    MirtSkyState*         d_sky = nullptr;
    size_t cap_spheres = 0, cap_mats = 0, cap_texels = 0;

    Tuning tuning;

    // per-launch state: every launch owns the dispenser word and the counter block of its event slot, so
    // launches of one context that overlap on different streams cannot disturb each other
    unsigned long long* d_counters = nullptr;      // [kEventPool][kNumCounters]
    uint32_t*           d_work_counter = nullptr;  // [kEventPool][kDispenserWords]: word 0 = the launch's dispenser; words kDispenserStride k = the 8 dispensers of a lane-per-pixel launch
    size_t              last_slot = 0;             // event slot of the last launch (its counters feed MirtStats)
    hipEvent_t          ev_accum = nullptr;        // end of the last launch that adds into d_accum
    bool                accum_pending = false;
    hipStream_t         accum_stream = nullptr;    // the stream of the last launch that uses d_accum: an add, or a frame -- also one that only reads
                                                   // the sums, spp == 0 (nullptr: none since the reset).  What order_frame orders the next frame after.
    hipEvent_t          ev_order = nullptr;        // progressive frames that change streams: the next one waits for the last one (order_frame)
    uint32_t*           d_out = nullptr;     // scratch framebuffer for host-output renders
    size_t              cap_out = 0;
    unsigned long long* d_accum = nullptr;   // progressive accumulation: [pixels][3] exact sums
    size_t              cap_accum = 0;
    uint64_t            accum_pixels = 0;
    uint32_t            accum_samples = 0;
    uint32_t            accum_width = 0, accum_rows = 0;

    MirtStats stats{};
    bool      stats_counted = false;
    char      last_kernel[128] = "";

    // MIRT_SCENE_HBM scene (mirt_ctx_set_scene_ex): the tables stay in device memory, the nearest hit runs through a BVH
    bool           hbm = false;
    unsigned char* d_bvh = nullptr;          // one allocation: nodes | test records | original ids (mirt_bvh.h)
    size_t         cap_bvh = 0;
    size_t         bvh_off_recs = 0, bvh_off_ids = 0;
    uint32_t       bvh_root = 0, bvh_n_always = 0;
    float          bvh_centre[3] = {}, bvh_radius = 0.0f, bvh_rmax = 0.0f;
    MirtBvhPlan    bvh_plan{};               // of the tree in d_bvh, whichever builder made it (mirt_ctx_bvh_info)
    bool           bvh_on_device = false;    // MIRT_SCENE_BVH_DEVICE built it
    mirt::BvhDeviceScratch bvh_scratch;      // the device builder's temporary storage: grows, never shrinks
    // mirt_ctx_update_spheres*: the schedule of a refit (prepared at the scene's first update) and the updates since the scene was set
    std::vector<uint32_t> bvh_levels;        // a device-built tree's level ranges, kept from its build
    mirt::BvhRefit bvh_refit;
    mirt::BvhDeviceScratch bvh_stage;        // the records of a host update on their way to the scatter: grows with the largest count
    uint32_t       bvh_refits = 0;

    // mirt_ctx_trace_rays* (DESIGN.md 10.7): state of its own, so that a trace touches neither the launch ring nor MirtStats
    hipEvent_t          ev_trace_begin = nullptr, ev_trace_end = nullptr;   // around the last trace kernel, on its stream
    bool                trace_pending = false;     // ev_trace_end is recorded and nobody has waited for it yet
    bool                trace_timed = false, trace_counted = false;
    unsigned long long* d_trace_counters = nullptr;   // [kNumCounters] of the last counting trace
    unsigned char*      d_trace_rays = nullptr;    // staging of the host path: [n] MirtRay, [n] MirtRayHit
    unsigned char*      d_trace_hits = nullptr;
    size_t              cap_trace_rays = 0, cap_trace_hits = 0;
    MirtRayStats        trace_stats{};
    // MIRT_RAYS_SORT / MIRT_RADIANCE_SORT: codes, order and the sort's storage; grows, never shrinks; shared by all sorted launches
    mirt::BvhDeviceScratch ray_sort;
    size_t              ray_sort_off_order = 0;    // of the last sorted launch: its permutation in ray_sort.d, [ray_sort_n] uint32
    uint32_t            ray_sort_n = 0;
    bool                ray_sort_any = false;      // a sorted launch has been queued on this context

    // mirt_ctx_adapt_* (DESIGN.md 10.12): the records and the select stage's storage, state of their own like the ray queries'; both grow, never shrink
    unsigned char*      d_adapt = nullptr;         // [adapt_pixels] MirtAdaptPixel
    size_t              cap_adapt = 0;
    unsigned char*      d_adapt_sel = nullptr;     // head {count, spp of a run's step, u64 samples added} | list [pixels] u32 | block counts [ceil(pixels / 256)] u32 | flags [pixels] u8 | run log
    size_t              cap_adapt_sel = 0;
    size_t              adapt_off_counts = 0, adapt_off_flags = 0;
    size_t              adapt_off_log = 0;         // behind the flags, 8-byte aligned: the run log, MIRT_ADAPT_RUN_MAX_STEPS x MirtAdaptRunStep (10.14)
    uint32_t            adapt_run_steps = 0;       // max_steps of the last run since the reset; 0: none
    uint64_t            adapt_pixels = 0;
    uint32_t            adapt_width = 0, adapt_rows = 0;
    uint32_t            adapt_steps = 0;           // since the reset
    hipEvent_t          ev_adapt_begin = nullptr, ev_adapt_end = nullptr;   // around the last step (select through render), on its stream
    bool                adapt_pending = false;     // ev_adapt_end is recorded and nobody has waited for it yet
    bool                adapt_timed = false;
    double              adapt_ms = 0.0;

    // mirt_ctx_denoise* (DESIGN.md 10.17): two colour planes and one guide plane, 16 bytes per pixel each; grows, never shrinks; shared by all denoise launches
    unsigned char*      d_denoise = nullptr;
    size_t              cap_denoise = 0;
};

extern "C" {

uint32_t mirt_version(void) { return (MIRT_VERSION_MAJOR << 16) | (MIRT_VERSION_MINOR << 8) | MIRT_VERSION_PATCH; }

const char* mirt_last_error(void) { return g_err; }

const char* mirt_status_string(int status)
{
    switch (status) {
    case MIRT_OK: return "MIRT_OK";
    case MIRT_ERR_MAX_SAMPLES_MULTIPLE: return "MIRT_ERR_MAX_SAMPLES_MULTIPLE";
    case MIRT_ERR_VIEWPORT_SIZE: return "MIRT_ERR_VIEWPORT_SIZE";
    case MIRT_ERR_VFOV_RANGE: return "MIRT_ERR_VFOV_RANGE";
    case MIRT_ERR_APERTURE_RANGE: return "MIRT_ERR_APERTURE_RANGE";
    case MIRT_ERR_FOCUS_DISTANCE: return "MIRT_ERR_FOCUS_DISTANCE";
    case MIRT_ERR_SKY: return "MIRT_ERR_SKY";
    case MIRT_ERR_NULL_POINTER: return "MIRT_ERR_NULL_POINTER";
    case MIRT_ERR_SPP_ZERO: return "MIRT_ERR_SPP_ZERO";
    case MIRT_ERR_BAD_MODE: return "MIRT_ERR_BAD_MODE";
    case MIRT_ERR_BAD_ROWS: return "MIRT_ERR_BAD_ROWS";
    case MIRT_ERR_MATERIAL_INDEX: return "MIRT_ERR_MATERIAL_INDEX";
    case MIRT_ERR_TEXEL_RANGE: return "MIRT_ERR_TEXEL_RANGE";
    case MIRT_ERR_OUT_BUFFER: return "MIRT_ERR_OUT_BUFFER";
    case MIRT_ERR_NO_SCENE: return "MIRT_ERR_NO_SCENE";
    case MIRT_ERR_SCENE_TOO_LARGE: return "MIRT_ERR_SCENE_TOO_LARGE";
    case MIRT_ERR_FRAME_SPP: return "MIRT_ERR_FRAME_SPP";
    case MIRT_ERR_NO_DEVICE: return "MIRT_ERR_NO_DEVICE";
    case MIRT_ERR_HIP: return "MIRT_ERR_HIP";
    case MIRT_ERR_ALLOC: return "MIRT_ERR_ALLOC";
    case MIRT_ERR_IMAGE_DECODE: return "MIRT_ERR_IMAGE_DECODE";
    case MIRT_ERR_SPP_RANGE: return "MIRT_ERR_SPP_RANGE";
    default: return "MIRT_ERR_UNKNOWN";
    }
}

// Angle::degrees / as_degrees (reference src/raytracer/angle.rs:8-22)
float mirt_degrees_to_radians(float degrees) { return degrees * kRustPi / 180.0f; }
float mirt_radians_to_degrees(float radians) { return radians * 180.0f / kRustPi; }

// RenderParams::validate (reference src/raytracer/mod.rs:450-484), same order of checks
int mirt_validate_render_params(const MirtCamera* camera, const MirtSamplingParams* sampling, uint32_t w, uint32_t h)
{
    if (!camera || !sampling) return fail(MIRT_ERR_NULL_POINTER, "camera/sampling is null");
    if (sampling->num_samples_per_pixel == 0)
        return fail(MIRT_ERR_SPP_ZERO, "num_samples_per_pixel is zero");
    if (sampling->max_samples_per_pixel % sampling->num_samples_per_pixel != 0)
        return fail(MIRT_ERR_MAX_SAMPLES_MULTIPLE, "max_samples_per_pixel (%u) is not a multiple of num_samples_per_pixel (%u)",
                    sampling->max_samples_per_pixel, sampling->num_samples_per_pixel);
    if (w == 0 || h == 0) return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", w, h);
    const float lo = mirt_degrees_to_radians(0.0f), hi = mirt_degrees_to_radians(90.0f);
    if (!(camera->vfov_radians >= lo && camera->vfov_radians <= hi))
        return fail(MIRT_ERR_VFOV_RANGE, "vfov must be between 0..=90 degrees");
    if (!(camera->aperture >= 0.0f && camera->aperture <= 1.0f))
        return fail(MIRT_ERR_APERTURE_RANGE, "aperture must be between 0..=1");
    if (camera->focus_distance < 0.0f)
        return fail(MIRT_ERR_FOCUS_DISTANCE, "focus_distance must be greater than zero");
    return MIRT_OK;
}

// GpuCamera::new (reference src/raytracer/mod.rs:700-741)
int mirt_camera_new(const MirtCamera* camera, uint32_t vw, uint32_t vh, MirtGpuCamera* out)
{
    if (!camera || !out) return fail(MIRT_ERR_NULL_POINTER, "camera/out is null");
    if (vw == 0 || vh == 0) return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", vw, vh);
    const float lens_radius = 0.5f * camera->aperture;
    const float aspect = (float)vw / (float)vh;
    const float half_height = camera->focus_distance * std::tan(0.5f * camera->vfov_radians);
    const float half_width = aspect * half_height;
    const V3 eye{ camera->eye_pos[0], camera->eye_pos[1], camera->eye_pos[2] };
    const V3 w = normalize3(V3{ camera->eye_dir[0], camera->eye_dir[1], camera->eye_dir[2] });
    const V3 v = normalize3(V3{ camera->up[0], camera->up[1], camera->up[2] });
    const V3 u = cross3(w, v);
    const V3 llc = sub3(sub3(add3(eye, scale3(camera->focus_distance, w)), scale3(half_width, u)), scale3(half_height, v));
    const V3 horizontal = scale3(2.0f * half_width, u);
    const V3 vertical = scale3(2.0f * half_height, v);
    std::memset(out, 0, sizeof *out);
    out->eye[0] = eye.x; out->eye[1] = eye.y; out->eye[2] = eye.z;
    out->horizontal[0] = horizontal.x; out->horizontal[1] = horizontal.y; out->horizontal[2] = horizontal.z;
    out->vertical[0] = vertical.x; out->vertical[1] = vertical.y; out->vertical[2] = vertical.z;
    out->u[0] = u.x; out->u[1] = u.y; out->u[2] = u.z;
    out->v[0] = v.x; out->v[1] = v.y; out->v[2] = v.z;
    out->lens_radius = lens_radius;
    out->lower_left_corner[0] = llc.x; out->lower_left_corner[1] = llc.y; out->lower_left_corner[2] = llc.z;
    return MIRT_OK;
}

// camera_orientation + FlyCameraController::renderer_camera (reference src/fly_camera.rs:52-64, 227-241)
int mirt_camera_from_fly_pose(const float position[3], float yaw, float pitch, float vfov_degrees, float aperture,
                              float focus_distance, MirtCamera* out)
{
    if (!position || !out) return fail(MIRT_ERR_NULL_POINTER, "position/out is null");
    const V3 forward = normalize3(V3{ std::cos(yaw) * std::cos(pitch), std::sin(pitch), std::sin(yaw) * std::cos(pitch) });
    const V3 right = cross3(forward, V3{ 0.0f, 1.0f, 0.0f });
    const V3 up = cross3(right, forward);
    out->eye_pos[0] = position[0]; out->eye_pos[1] = position[1]; out->eye_pos[2] = position[2];
    out->eye_dir[0] = forward.x; out->eye_dir[1] = forward.y; out->eye_dir[2] = forward.z;
    out->up[0] = up.x; out->up[1] = up.y; out->up[2] = up.z;
    out->vfov_radians = mirt_degrees_to_radians(vfov_degrees);
    out->aperture = aperture;
    out->focus_distance = focus_distance;
    return MIRT_OK;
}

uint32_t mirt_params_out_rows(const MirtParams* params) { return out_rows(params); }

uint32_t mirt_params_out_row_index(const MirtParams* p, uint32_t i)
{
    uint32_t rb, re;
    if (!p || !rows_valid(p, &rb, &re) || i >= out_rows(p)) return UINT32_MAX;
    if (p->tile_rows == 0 || p->n_parts <= 1) return rb + i;
    const uint32_t t = p->part + (i / p->tile_rows) * p->n_parts;
    return rb + t * p->tile_rows + i % p->tile_rows;
}

int mirt_grid_plan(const MirtSphere* spheres, uint32_t n_spheres, uint64_t lds_bytes_per_block, MirtGridPlan* out)
{
    if (!out || (n_spheres && !spheres)) return fail(MIRT_ERR_NULL_POINTER, "spheres/out is null");
    *out = MirtGridPlan{};
    const size_t lds = lds_bytes_per_block ? (size_t)lds_bytes_per_block : (size_t)160 * 1024;
    double f = 0.0;
    const Tuning tune = read_tuning();                 // the experiment knobs MIRT_GRID_CELL / MIRT_GRID_BIG apply as in mirt_ctx_create
    const std::vector<unsigned char> grid = plan_grid(spheres, n_spheres, tune.grid_cell, tune.grid_big, lds, &f);
    if (grid.empty() || n_spheres > 4095u || kx::scene_lds_bytes_grid(n_spheres, true) + grid.size() > mirt::kMaxLdsBytes) return MIRT_OK;
    const mirt::GridHeader* gh = reinterpret_cast<const mirt::GridHeader*>(grid.data());
    out->cell_factor = (float)f;
    out->blob_bytes = (uint32_t)grid.size();
    out->n_cells = gh->dims[0] * gh->dims[1] * gh->dims[2];
    out->n_entries = gh->n_entries;
    out->n_big = gh->n_big;
    const size_t beside = kx::scene_lds_bytes_grid(n_spheres, true) + grid.size();
    out->pool_slots = beside < lds ? kx::pool_config_grid(lds - beside, false).slots : 0u;
    return MIRT_OK;
}

int mirt_bvh_pool_plan(uint32_t max_depth, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtBvhPoolPlan* out)
{
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out is null");
    *out = MirtBvhPoolPlan{};
    if (max_depth > MIRT_BVH_MAX_DEPTH) return fail(MIRT_ERR_BAD_ROWS, "max_depth %u exceeds MIRT_BVH_MAX_DEPTH (%u)", max_depth, (unsigned)MIRT_BVH_MAX_DEPTH);
    *out = plan_bvh_pool(max_depth, hosek != 0u, lds_bytes_per_cu ? lds_bytes_per_cu : (uint64_t)160 * 1024, 0u, 0u);
    return MIRT_OK;
}

int mirt_adapt_pool_plan(uint32_t max_depth, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtBvhPoolPlan* out)
{
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out is null");
    *out = MirtBvhPoolPlan{};
    if (max_depth > MIRT_BVH_MAX_DEPTH) return fail(MIRT_ERR_BAD_ROWS, "max_depth %u exceeds MIRT_BVH_MAX_DEPTH (%u)", max_depth, (unsigned)MIRT_BVH_MAX_DEPTH);
    *out = plan_bvh_pool(max_depth, hosek != 0u, lds_bytes_per_cu ? lds_bytes_per_cu : (uint64_t)160 * 1024, 0u, mirt::kAdaptPoolExtraBytes);
    return MIRT_OK;
}

int mirt_adapt_lds_plan(uint32_t n_spheres, uint32_t n_materials, uint32_t grid_bytes, uint32_t hosek, uint64_t lds_bytes_per_cu, MirtAdaptLdsPlan* out)
{
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out is null");
    *out = mirt::plan_adapt_lds(n_spheres, n_materials, grid_bytes, hosek != 0u, lds_bytes_per_cu ? lds_bytes_per_cu : (uint64_t)160 * 1024);
    return MIRT_OK;
}

int mirt_adapt_lds_groups(uint32_t count, uint32_t spp, uint32_t grid_waves, uint32_t* out_log2)
{
    if (!out_log2) return fail(MIRT_ERR_NULL_POINTER, "out_log2 is null");
    if (spp == 0u || (spp & 1u) || spp > MIRT_MAX_SPP_PER_CALL) return fail(MIRT_ERR_SPP_RANGE, "spp %u: a step's size is even, 2 .. %u", spp, (unsigned)MIRT_MAX_SPP_PER_CALL);
    if (grid_waves == 0u) return fail(MIRT_ERR_BAD_ROWS, "grid_waves is 0");
    *out_log2 = mirt::adapt_lds_groups(count, spp, grid_waves);
    return MIRT_OK;
}

int mirt_ctx_create(int device, MirtContext** out)
{
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MIRT_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(MIRT_ERR_NO_DEVICE, "device %d out of range (0..%d)", device, n - 1);
    MirtContext* c = new (std::nothrow) MirtContext();
    if (!c) return fail(MIRT_ERR_ALLOC, "out of host memory");
    c->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < kEventPool && e == hipSuccess; ++i) {
        hipEvent_t a = nullptr, b = nullptr;
        e = hipEventCreate(&a);
        if (e == hipSuccess) e = hipEventCreate(&b);
        if (a) c->ev_begin.push_back(a);
        if (b) c->ev_end.push_back(b);
        hipEvent_t z = nullptr;
        if (e == hipSuccess) e = hipEventCreateWithFlags(&z, hipEventDisableTiming);
        if (z) c->ev_zeroed.push_back(z);
    }
    c->slot_busy.assign(kEventPool, 0);
    c->slot_zeroing.assign(kEventPool, 0);
    c->slot_dirty.assign(kEventPool, 0);
    c->slot_zero_event.assign(kEventPool, 0);
    c->slot_timed.assign(kEventPool, 0);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->zero_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_accum, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&c->ev_trace_begin);
    if (e == hipSuccess) e = hipEventCreate(&c->ev_trace_end);
    if (e == hipSuccess) e = hipMalloc(&c->d_trace_counters, sizeof(unsigned long long) * mirt::kNumCounters);
    if (e == hipSuccess) e = hipMalloc(&c->d_sky, sizeof(MirtSkyState));
    if (e == hipSuccess) e = hipMalloc(&c->d_counters, sizeof(unsigned long long) * mirt::kNumCounters * kEventPool);
    if (e == hipSuccess) e = hipMalloc(&c->d_work_counter, sizeof(uint32_t) * kEventPool * kDispenserWords);
    if (e == hipSuccess) e = hipMemset(c->d_work_counter, 0, sizeof(uint32_t) * kEventPool * kDispenserWords);     // see retire_slots / launch_render
    if (e != hipSuccess) {
        const int rc = fail(MIRT_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        mirt_ctx_destroy(c);
        return rc;
    }
    c->cu_count = prop.multiProcessorCount;
    c->lds_per_block = prop.sharedMemPerBlock;            // 160 KiB on gfx950
    c->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : prop.sharedMemPerBlock;
    c->tuning = read_tuning();
    c->timing = c->tuning.timing != 0;
    *out = c;
    return MIRT_OK;
}

void mirt_ctx_destroy(MirtContext* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->zero_stream) (void)hipStreamSynchronize(c->zero_stream);
    if (c->frame_stream_b) (void)hipStreamSynchronize(c->frame_stream_b);
    if (!c->untimed_streams.empty()) (void)hipDeviceSynchronize();      // launches without an event may still read the tables freed below
    if (c->trace_pending) (void)hipEventSynchronize(c->ev_trace_end);    // a trace on a caller stream reads them too
    if (c->adapt_pending) (void)hipEventSynchronize(c->ev_adapt_end);    // ... and so does an adaptive step
    (void)hipFree(c->d_adapt); (void)hipFree(c->d_adapt_sel); (void)hipFree(c->d_denoise);
    if (c->ev_adapt_begin) (void)hipEventDestroy(c->ev_adapt_begin);
    if (c->ev_adapt_end) (void)hipEventDestroy(c->ev_adapt_end);
    (void)hipFree(c->d_trace_counters); (void)hipFree(c->d_trace_rays); (void)hipFree(c->d_trace_hits); (void)hipFree(c->ray_sort.d);
    if (c->ev_trace_begin) (void)hipEventDestroy(c->ev_trace_begin);
    if (c->ev_trace_end) (void)hipEventDestroy(c->ev_trace_end);
    (void)hipFree(c->d_spheres); (void)hipFree(c->d_mats); (void)hipFree(c->d_pmats); (void)hipFree(c->d_grid); (void)hipFree(c->d_shade); (void)hipFree(c->d_bvh); (void)hipFree(c->bvh_scratch.d); (void)hipFree(c->bvh_stage.d); (void)hipFree(c->d_texels);
    (void)hipFree(c->d_sky); (void)hipFree(c->d_counters); (void)hipFree(c->d_work_counter); (void)hipFree(c->d_out); (void)hipFree(c->d_accum);
    for (hipEvent_t ev : c->ev_begin) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->ev_end) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : c->ev_zeroed) (void)hipEventDestroy(ev);
    if (c->zero_stream) (void)hipStreamDestroy(c->zero_stream);
    if (c->frame_stream_b) (void)hipStreamDestroy(c->frame_stream_b);
    if (c->ev_accum) (void)hipEventDestroy(c->ev_accum);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Which scatter routines can a path meet?  (decides the path-traced schedule; the pool kernel numbers the routines present densely
// so that scenes with <= 3 of them run a 4-queue build.)  seen: bit min(GpuMaterial.id, 4) of every sphere's material;
// routine_queue: routine id -> queue of the pool kernel.
static void set_routines(MirtContext* c, uint32_t seen, uint32_t routine_queue[5])
{
    c->n_shading_routines = (uint32_t)__builtin_popcount(seen);
    uint32_t q = 0;
    for (uint32_t r = 0; r < 5; ++r) if (seen & (1u << r)) { routine_queue[r] = q; c->queue_routine[q] = r; ++q; }
    for (uint32_t r = 0; r < 5; ++r) if (!(seen & (1u << r))) { routine_queue[r] = q; c->queue_routine[q] = r; ++q; }
}

// the tree build_bvh_device has just left in c->d_bvh becomes the context's
static void adopt_device_tree(MirtContext* c, mirt::BvhDeviceResult* r)
{
    c->bvh_off_recs = r->off_recs;
    c->bvh_off_ids = r->off_ids;
    c->bvh_root = r->root;
    c->bvh_n_always = r->plan.n_always;
    for (int k = 0; k < 3; ++k) c->bvh_centre[k] = r->centre[k];
    c->bvh_radius = r->radius;
    c->bvh_rmax = r->r_max;
    c->bvh_plan = r->plan;
    c->bvh_on_device = true;
    c->bvh_levels.swap(r->level_first);
}

// mirt_ctx_set_scene (hbm = false) and mirt_ctx_set_scene_ex (hbm = true: MIRT_SCENE_HBM; bvh_device: | MIRT_SCENE_BVH_DEVICE)
static int set_scene(MirtContext* c, const MirtScene* s, bool hbm, bool bvh_device = false)
{
    if (!c || !s || !s->camera) return fail(MIRT_ERR_NULL_POINTER, "ctx/scene/camera is null");
    if (s->n_spheres && !s->spheres) return fail(MIRT_ERR_NULL_POINTER, "spheres is null");
    if (s->n_materials && !s->materials) return fail(MIRT_ERR_NULL_POINTER, "materials is null");
    if (s->n_texels && !s->texels) return fail(MIRT_ERR_NULL_POINTER, "texels is null");
    if (hbm && s->n_spheres > MIRT_SCENE_HBM_MAX_SPHERES)            // before any sphere is read
        return fail(MIRT_ERR_SCENE_TOO_LARGE, "%u spheres exceed MIRT_SCENE_HBM_MAX_SPHERES (%u)", s->n_spheres, (unsigned)MIRT_SCENE_HBM_MAX_SPHERES);
    // The flat kernels stage spheres AND materials in LDS; the grid build (path-traced mode, many spheres)
    // only the spheres + the grid.  A scene is accepted if at least one of the two layouts fits.
    const bool fits_flat = !hbm && kx::scene_lds_bytes(s->n_spheres, s->n_materials, true, true) <= mirt::kMaxLdsBytes;
    // The cell size trades sphere tests against cells walked AND against LDS: the blob shares the CU's 160 KB with the path pools,
    // and a pool geometry lost to a large cell table costs more than finer cells bring (RTIOW: cell = 2 median radii drops the
    // pools from 152 to 128 slots per wave and the frame from 13.2 to 19.7 ms): plan_grid.
    double grid_factor = 0.0;
    std::vector<unsigned char> grid;
    if (!hbm) grid = plan_grid(s->spheres, s->n_spheres, c->tuning.grid_cell, c->tuning.grid_big, c->lds_per_block, &grid_factor);
    const bool fits_grid = !grid.empty() && s->n_spheres <= 4095u &&
                           kx::scene_lds_bytes_grid(s->n_spheres, true) + grid.size() <= mirt::kMaxLdsBytes;   // camera (+ sky) + the blob
    if (!hbm && !fits_flat && !fits_grid)
        return fail(MIRT_ERR_SCENE_TOO_LARGE, "%u spheres + %u materials exceed the %u-byte LDS budget", s->n_spheres,
                    s->n_materials, mirt::kMaxLdsBytes);
    // MIRT_SCENE_HBM: the BVH (host, mirt_bvh.cpp), built before the context's scene is touched
    // (MIRT_SCENE_BVH_DEVICE: only the always-tested list here; the tree is built on the device once the spheres are there)
    mirt::BvhBuild bvh;
    std::vector<uint32_t> bvh_always;
    mirt::BvhDeviceResult dev_bvh;
    if (hbm && !bvh_device) {
        const int rc = mirt::build_bvh(s->spheres, s->n_spheres, &bvh);
        if (rc != MIRT_OK) return rc;
    } else if (hbm) {
        const auto t0 = std::chrono::steady_clock::now();
        try {
            bvh_always = mirt::bvh_always_list(s->spheres, s->n_spheres);
        } catch (const std::bad_alloc&) {
            return fail(MIRT_ERR_ALLOC, "out of host memory listing the always-tested spheres of %u", s->n_spheres);
        }
        dev_bvh.always_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    HIP_TRY(hipSetDevice(c->device));
    // Failure-atomic: from here until the last copy has succeeded the context holds NO scene, so an allocation or
    // copy that fails half-way leaves render calls answering MIRT_ERR_NO_SCENE instead of launching on freed or
    // half-written tables.
    c->have_scene = false;
    c->fits_flat = fits_flat;
    c->hbm = hbm;
    c->bvh_refits = 0;
    c->bvh_refit.ready = false;

    // mode-specific validity is decided here once and reported by the render call that needs it
    // (the spheres first, then the materials -- whose verdict mirt_ctx_set_spheres* keeps)
    c->pt_scene_status = MIRT_OK;
    for (uint32_t i = 0; i < s->n_spheres && c->pt_scene_status == MIRT_OK; ++i)
        if (s->spheres[i].material_idx >= s->n_materials) c->pt_scene_status = MIRT_ERR_MATERIAL_INDEX;
    c->pt_materials_status = MIRT_OK;
    for (uint32_t i = 0; i < s->n_materials && c->pt_materials_status == MIRT_OK; ++i) {
        const MirtMaterial& m = s->materials[i];
        if ((m.id == 0 || m.id == 1 || m.id == 3) && !desc_ok(m.desc1, s->n_texels)) c->pt_materials_status = MIRT_ERR_TEXEL_RANGE;
        if (m.id == 3 && !desc_ok(m.desc2, s->n_texels)) c->pt_materials_status = MIRT_ERR_TEXEL_RANGE;
    }
    if (c->pt_scene_status == MIRT_OK) c->pt_scene_status = c->pt_materials_status;
    uint32_t routine_queue[5] = {0, 1, 2, 3, 4};    // routine id -> queue of the pool kernel
    {
        uint32_t seen = 0;
        for (uint32_t i = 0; i < s->n_spheres; ++i) {
            const uint32_t mi = s->spheres[i].material_idx;
            if (mi < s->n_materials) { const uint32_t id = s->materials[mi].id; seen |= 1u << (id < 4u ? id : 4u); }
        }
        set_routines(c, seen, routine_queue);
    }
    // layer.rs:345-349 reads material_data[2] on every primary hit
    c->parity_materials_status = s->n_materials < 3 ? MIRT_ERR_MATERIAL_INDEX : !desc_ok(s->materials[2].desc1, s->n_texels) ? MIRT_ERR_TEXEL_RANGE : MIRT_OK;
    c->parity_scene_status = s->n_spheres > 0 ? c->parity_materials_status : MIRT_OK;

    std::vector<mirt::PreparedSphere> prep(s->n_spheres);
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const MirtSphere& in = s->spheres[i];
        mirt::PreparedSphere& o = prep[i];
        o.cx = in.center[0]; o.cy = in.center[1]; o.cz = in.center[2];
        o.rr = in.radius * in.radius;
        o.inv_r = 1.0f / in.radius;
        o.radius = in.radius;
        o.material_idx = in.material_idx;
        o.op = routine_queue[(in.material_idx < s->n_materials && s->materials[in.material_idx].id < 4u) ? s->materials[in.material_idx].id : 4u];
    }
    // PreparedMaterial: GpuMaterial + 1/x + the texel of every 1x1 texture (see mirt_kernels.h)
    std::vector<mirt::PreparedMaterial> pmats(s->n_materials);
    std::vector<unsigned char> mat_has_image(s->n_materials, 0);     // a texture larger than 1x1: what MIRT_FLAG_TEXEL_TILES caches in LDS
    for (uint32_t i = 0; i < s->n_materials; ++i) {
        const MirtMaterial& in = s->materials[i];
        mirt::PreparedMaterial& o = pmats[i];
        std::memset(&o, 0, sizeof o);
        o.id = in.id;
        o.x = in.x;
        o.inv_x = 1.0f / in.x;
        const MirtTextureDescriptor* d[2] = { &in.desc1, &in.desc2 };
        for (int k = 0; k < 2; ++k) {
            uint32_t w = d[k]->width, h = d[k]->height, off = d[k]->offset;
            if (w == 1 && h == 1 && (uint64_t)off < s->n_texels) {
                o.flags |= (1u << k);
                o.tex[k][0] = s->texels[3 * (size_t)off + 0];
                o.tex[k][1] = s->texels[3 * (size_t)off + 1];
                o.tex[k][2] = s->texels[3 * (size_t)off + 2];
                std::memcpy(&o.tex[k][3], &off, 4);
            } else {
                if ((uint64_t)w * h > 1u) mat_has_image[i] = 1;
                std::memcpy(&o.tex[k][0], &w, 4);
                std::memcpy(&o.tex[k][1], &h, 4);
                std::memcpy(&o.tex[k][2], &off, 4);
            }
        }
    }
    if (!grid.empty()) {                         // routine queue of every sphere, for the grid builds (GridHeader.off_ops)
        const mirt::GridHeader* gh = reinterpret_cast<const mirt::GridHeader*>(grid.data());
        for (uint32_t i = 0; i < s->n_spheres; ++i) {            // the ROUTINE itself, min(GpuMaterial.id, 4): what the scatter step switches on
            const uint32_t mi = s->spheres[i].material_idx;
            grid[gh->off_ops + i] = (unsigned char)((mi < s->n_materials && s->materials[mi].id < 4u) ? s->materials[mi].id : 4u);
        }
    }
    // grid builds: sphere centre, 1/r and a copy of the sphere's material in one 64-byte record (mirt_kernels.h: ShadeRec)
    std::vector<mirt::ShadeRec> shade;
    if (fits_grid && s->n_materials) {
        shade.resize(s->n_spheres);
        for (uint32_t i = 0; i < s->n_spheres; ++i) {
            const uint32_t mi = prep[i].material_idx < s->n_materials ? prep[i].material_idx : 0u;   // out of range: pt_scene_status refuses the launch
            const mirt::PreparedMaterial& pm = pmats[mi];
            float fl, idf;
            std::memcpy(&fl, &pm.flags, 4);
            std::memcpy(&idf, &pm.id, 4);
            shade[i] = mirt::ShadeRec{ { prep[i].inv_r, pm.x, pm.inv_x, fl }, { pm.tex[0][0], pm.tex[0][1], pm.tex[0][2], pm.tex[0][3] },
                                       { pm.tex[1][0], pm.tex[1][1], pm.tex[1][2], pm.tex[1][3] }, { prep[i].cx, prep[i].cy, prep[i].cz, idf } };
        }
    }
    int rc;
    if (!shade.empty() && (rc = ensure_capacity(&c->d_shade, &c->cap_shade, shade.size())) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_pmats, &c->cap_pmats, (size_t)s->n_materials)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_spheres, &c->cap_spheres, (size_t)s->n_spheres)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_mats, &c->cap_mats, (size_t)s->n_materials)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_texels, &c->cap_texels, (size_t)s->n_texels * 3)) != MIRT_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());      // renders may be in flight on caller streams (mirt_ctx_render_device)
    const auto t_upload = std::chrono::steady_clock::now();
    c->cam = *s->camera;
    if (s->n_spheres) HIP_TRY(hipMemcpy(c->d_spheres, prep.data(), prep.size() * sizeof(mirt::PreparedSphere), hipMemcpyHostToDevice));
    if (s->n_materials) HIP_TRY(hipMemcpy(c->d_mats, s->materials, (size_t)s->n_materials * sizeof(MirtMaterial), hipMemcpyHostToDevice));
    if (s->n_materials) HIP_TRY(hipMemcpy(c->d_pmats, pmats.data(), pmats.size() * sizeof(mirt::PreparedMaterial), hipMemcpyHostToDevice));
    if (s->n_texels) HIP_TRY(hipMemcpy(c->d_texels, s->texels, (size_t)s->n_texels * 3 * sizeof(float), hipMemcpyHostToDevice));
    if (!shade.empty()) HIP_TRY(hipMemcpy(c->d_shade, shade.data(), shade.size() * sizeof(mirt::ShadeRec), hipMemcpyHostToDevice));
    c->have_shade = !shade.empty();
    {
        c->grid_bytes = fits_grid ? (uint32_t)grid.size() : 0u;
        c->grid_packable = false;
        c->grid_flat_y = false;
        if (fits_grid) {
            const mirt::GridHeader* gh = reinterpret_cast<const mirt::GridHeader*>(grid.data());
            c->grid_packable = gh->dims[0] * gh->dims[1] * gh->dims[2] <= mirt::kGridMaxCells;      // a parked walk keeps its linear cell index (16 bit)
            c->grid_flat_y = gh->dims[1] == 1u && c->tuning.grid_flat_y != 0;
        }
        if (fits_grid) {
            if ((rc = ensure_capacity(&c->d_grid, &c->cap_grid, grid.size())) != MIRT_OK) return rc;
            HIP_TRY(hipMemcpy(c->d_grid, grid.data(), grid.size(), hipMemcpyHostToDevice));
        }
    }
    c->have_sky = s->sky != nullptr;
    if (s->sky) HIP_TRY(hipMemcpy(c->d_sky, s->sky, sizeof(MirtSkyState), hipMemcpyHostToDevice));
    c->n_spheres = s->n_spheres;
    c->n_mats = s->n_materials;
    c->n_texels = s->n_texels;
    for (uint32_t i = 0; i < 3; ++i)
        for (int k = 0; k < 4; ++k) c->sph3[4 * i + k] = (s->n_spheres == 3) ? (&prep[i].cx)[k] : 0.0f;
    c->has_image_texture = false;                // ... on a material some sphere uses
    for (uint32_t i = 0; i < s->n_spheres; ++i)
        if (s->spheres[i].material_idx < s->n_materials && mat_has_image[s->spheres[i].material_idx]) c->has_image_texture = true;
    if (hbm && bvh_device) {                     // the tree from the prepared spheres just uploaded, on the context's stream; synchronous
        const double upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_upload).count();
        if ((rc = mirt::build_bvh_device(bvh_always, s->n_spheres, c->d_spheres, c->stream, &c->bvh_scratch, &c->d_bvh, &c->cap_bvh, &dev_bvh)) != MIRT_OK) return rc;
        adopt_device_tree(c, &dev_bvh);
        if (std::getenv("MIRT_BVH_TIMING"))       // tools/hbm_scene_rates.py: the parts of a device build
            std::fprintf(stderr, "mirt_bvh_device: n=%u always_ms=%.3f upload_ms=%.3f kernels_ms=%.3f levels=%u\n", s->n_spheres, dev_bvh.always_ms,
                         upload_ms, dev_bvh.kernels_ms, dev_bvh.levels);
    } else if (hbm) {                            // nodes | records | ids, each 16-byte aligned
        const size_t nb = bvh.nodes.size() * sizeof(mirt::BvhNode), rb = bvh.recs.size() * sizeof(float), ib = bvh.ids.size() * sizeof(uint32_t);
        c->bvh_off_recs = nb;
        c->bvh_off_ids = nb + rb;
        if ((rc = ensure_capacity(&c->d_bvh, &c->cap_bvh, nb + rb + ib + 16)) != MIRT_OK) return rc;
        if (nb) HIP_TRY(hipMemcpy(c->d_bvh, bvh.nodes.data(), nb, hipMemcpyHostToDevice));
        if (rb) HIP_TRY(hipMemcpy(c->d_bvh + c->bvh_off_recs, bvh.recs.data(), rb, hipMemcpyHostToDevice));
        if (ib) HIP_TRY(hipMemcpy(c->d_bvh + c->bvh_off_ids, bvh.ids.data(), ib, hipMemcpyHostToDevice));
        c->bvh_root = bvh.root;
        c->bvh_n_always = bvh.n_always;
        for (int k = 0; k < 3; ++k) c->bvh_centre[k] = bvh.centre[k];
        c->bvh_radius = bvh.radius;
        c->bvh_rmax = bvh.r_max;
        c->bvh_plan = mirt::bvh_plan_of(bvh);
        c->bvh_on_device = false;
    }
    c->have_scene = true;
    return MIRT_OK;
}

int mirt_ctx_set_scene(MirtContext* c, const MirtScene* s) { return set_scene(c, s, false); }

int mirt_ctx_set_scene_ex(MirtContext* c, const MirtScene* s, uint32_t flags)
{
    if (flags & ~(uint32_t)(MIRT_SCENE_HBM | MIRT_SCENE_BVH_DEVICE)) return fail(MIRT_ERR_BAD_MODE, "unknown set_scene_ex flags 0x%x", flags);
    if ((flags & MIRT_SCENE_BVH_DEVICE) && !(flags & MIRT_SCENE_HBM))
        return fail(MIRT_ERR_BAD_MODE, "MIRT_SCENE_BVH_DEVICE needs MIRT_SCENE_HBM (flags 0x%x)", flags);
    return set_scene(c, s, (flags & MIRT_SCENE_HBM) != 0, (flags & MIRT_SCENE_BVH_DEVICE) != 0);
}

int mirt_ctx_bvh_info(MirtContext* c, MirtBvhInfo* out)
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    if (!c->have_scene || !c->hbm) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene");
    *out = MirtBvhInfo{};
    out->plan = c->bvh_plan;
    out->root = c->bvh_root;
    out->built_on_device = c->bvh_on_device ? 1u : 0u;
    for (int k = 0; k < 3; ++k) out->centre[k] = c->bvh_centre[k];
    out->radius = c->bvh_radius;
    out->r_max = c->bvh_rmax;
    return MIRT_OK;
}

int mirt_ctx_bvh_read(MirtContext* c, void* nodes, size_t nodes_bytes, float* recs, size_t recs_len, uint32_t* ids, size_t ids_len)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    if (!c->have_scene || !c->hbm) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene");
    const size_t nb = (size_t)c->bvh_plan.n_nodes * sizeof(mirt::BvhNode), n = c->n_spheres;
    if (nodes_bytes < nb || recs_len < 4 * n || ids_len < n)
        return fail(MIRT_ERR_OUT_BUFFER, "the tree needs %zu node bytes, %zu record floats and %zu ids", nb, 4 * n, n);
    if ((nb && !nodes) || (n && (!recs || !ids))) return fail(MIRT_ERR_NULL_POINTER, "nodes/recs/ids is null");
    HIP_TRY(hipSetDevice(c->device));
    if (nb) HIP_TRY(hipMemcpy(nodes, c->d_bvh, nb, hipMemcpyDeviceToHost));
    if (n) HIP_TRY(hipMemcpy(recs, c->d_bvh + c->bvh_off_recs, 16 * n, hipMemcpyDeviceToHost));
    if (n) HIP_TRY(hipMemcpy(ids, c->d_bvh + c->bvh_off_ids, 4 * n, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

// mirt_ctx_update_spheres (host pointer) and mirt_ctx_update_spheres_device
static int update_spheres(MirtContext* c, uint32_t first, uint32_t count, const void* spheres, bool on_device)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    if (count && !spheres) return fail(MIRT_ERR_NULL_POINTER, "spheres is null");
    if (!c->have_scene || !c->hbm) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene");
    if ((uint64_t)first + count > c->n_spheres)
        return fail(MIRT_ERR_BAD_ROWS, "spheres [%u, %llu) of a scene of %u", first, (unsigned long long)first + count, c->n_spheres);
    if (!count) return MIRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());      // renders may be in flight on caller streams; whatever produced a device source has finished too
    mirt::BvhTables t;
    t.d_bvh = c->d_bvh;
    t.off_recs = c->bvh_off_recs;
    t.off_ids = c->bvh_off_ids;
    t.d_prepared = c->d_spheres;
    t.n = c->n_spheres;
    t.n_nodes = c->bvh_plan.n_nodes;
    t.n_always = c->bvh_n_always;
    t.root = c->bvh_root;
    int rc;
    if (!c->bvh_refit.ready &&            // once per scene; nothing of the scene is written yet
        (rc = mirt::refit_prepare(&c->bvh_refit, t, c->bvh_on_device ? &c->bvh_levels : nullptr, c->stream, &c->bvh_scratch)) != MIRT_OK)
        return rc;
    // from the first write on, a failure leaves NO scene (as set_scene does)
    c->have_scene = false;
    float centre[3], radius, r_max, parts[3];
    const bool timed = std::getenv("MIRT_BVH_TIMING") != nullptr;
    if ((rc = mirt::refit_bvh_device(c->bvh_refit, t, c->stream, &c->bvh_scratch, &c->bvh_stage, first, count, spheres, on_device, centre, &radius, &r_max,
                                     timed ? parts : nullptr)) != MIRT_OK)
        return rc;
    if (c->n_spheres == 3) {              // the host copy of a three-sphere scene (RenderArgs.sph3): {centre, r * r} as the device computed them
        mirt::PreparedSphere prep[3];
        HIP_TRY(hipMemcpy(prep, c->d_spheres, sizeof prep, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < 3; ++i)
            for (int k = 0; k < 4; ++k) c->sph3[4 * i + k] = (&prep[i].cx)[k];
    }
    for (int k = 0; k < 3; ++k) c->bvh_centre[k] = centre[k];
    c->bvh_radius = radius;
    c->bvh_rmax = r_max;
    ++c->bvh_refits;
    c->have_scene = true;
    if (timed)                            // tools/hbm_scene_rates.py --update: the parts of an update
        std::fprintf(stderr, "mirt_bvh_refit: n=%u count=%u scatter_ms=%.3f refit_ms=%.3f bounds_ms=%.3f levels=%zu\n", c->n_spheres, count, parts[0],
                     parts[1], parts[2], c->bvh_refit.level_first.empty() ? (size_t)0 : c->bvh_refit.level_first.size() - 1);
    return MIRT_OK;
}

int mirt_ctx_update_spheres(MirtContext* c, uint32_t first, uint32_t count, const MirtSphere* spheres)
{
    return update_spheres(c, first, count, spheres, false);
}

int mirt_ctx_update_spheres_device(MirtContext* c, uint32_t first, uint32_t count, const void* d_spheres)
{
    return update_spheres(c, first, count, d_spheres, true);
}

uint32_t mirt_ctx_bvh_refits(const MirtContext* c) { return (c && c->have_scene && c->hbm) ? c->bvh_refits : 0u; }

// mirt_ctx_set_spheres (host pointer) and mirt_ctx_set_spheres_device: a new sphere table for the resident MIRT_SCENE_HBM scene, its
// materials, texels, camera and sky kept; afterwards the context is what set_scene_ex(HBM | BVH_DEVICE) of that scene leaves.
static int set_spheres(MirtContext* c, const void* spheres, uint32_t n, bool on_device)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    if (n && !spheres) return fail(MIRT_ERR_NULL_POINTER, "spheres is null");
    if (!c->have_scene || !c->hbm) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene");
    if (n > MIRT_SCENE_HBM_MAX_SPHERES)                              // before any sphere is read
        return fail(MIRT_ERR_SCENE_TOO_LARGE, "%u spheres exceed MIRT_SCENE_HBM_MAX_SPHERES (%u)", n, (unsigned)MIRT_SCENE_HBM_MAX_SPHERES);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());      // renders may be in flight on caller streams; whatever produced a device source has finished too
    const bool timed = std::getenv("MIRT_BVH_TIMING") != nullptr;
    int rc;
    const void* d_wire = spheres;
    if (!on_device && n) {                // host records go through the staging buffer of the host updates
        if ((rc = ensure_capacity(&c->bvh_stage.d, &c->bvh_stage.cap, 32ull * n)) != MIRT_OK) return rc;
        HIP_TRY(hipMemcpy(c->bvh_stage.d, spheres, 32ull * n, hipMemcpyHostToDevice));
        d_wire = c->bvh_stage.d;
    }
    // the census and the always-tested list write the builder scratch only -- where a refit keeps its tables
    c->bvh_refit.ready = false;
    mirt::SpheresCensus census;
    if ((rc = mirt::census_spheres_device(d_wire, n, c->d_mats, c->n_mats, c->stream, &c->bvh_scratch, timed, &census)) != MIRT_OK) return rc;
    // from the first write on, a failure leaves NO scene (as set_scene does)
    c->have_scene = false;
    c->bvh_refits = 0;
    c->bvh_levels.clear();
    c->pt_scene_status = census.bad_material_index ? MIRT_ERR_MATERIAL_INDEX : c->pt_materials_status;
    c->parity_scene_status = n > 0 ? c->parity_materials_status : MIRT_OK;
    uint32_t routine_queue[5] = {0, 1, 2, 3, 4};
    set_routines(c, census.routines_seen, routine_queue);
    c->has_image_texture = census.has_image_texture;
    if ((rc = ensure_capacity(&c->d_spheres, &c->cap_spheres, (size_t)n)) != MIRT_OK) return rc;
    float prepare_ms = 0.0f;
    if ((rc = mirt::prepare_spheres_device(d_wire, n, c->d_mats, c->n_mats, routine_queue, c->d_spheres, c->stream, timed ? &prepare_ms : nullptr)) != MIRT_OK)
        return rc;
    mirt::BvhDeviceResult dev_bvh;
    if ((rc = mirt::build_bvh_device(census.always, n, c->d_spheres, c->stream, &c->bvh_scratch, &c->d_bvh, &c->cap_bvh, &dev_bvh)) != MIRT_OK) return rc;
    c->n_spheres = n;
    for (int k = 0; k < 12; ++k) c->sph3[k] = 0.0f;
    if (n == 3) {                         // the host copy of a three-sphere scene (RenderArgs.sph3): {centre, r * r} as the device computed them
        mirt::PreparedSphere prep[3];
        HIP_TRY(hipMemcpy(prep, c->d_spheres, sizeof prep, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < 3; ++i)
            for (int k = 0; k < 4; ++k) c->sph3[4 * i + k] = (&prep[i].cx)[k];
    }
    adopt_device_tree(c, &dev_bvh);
    c->have_scene = true;
    if (timed)                            // tools/hbm_scene_rates.py --set-spheres: the parts of the call
        std::fprintf(stderr, "mirt_set_spheres: n=%u census_ms=%.3f always_ms=%.3f prepare_ms=%.3f kernels_ms=%.3f\n", n, census.census_ms,
                     census.always_ms, prepare_ms, dev_bvh.kernels_ms);
    return MIRT_OK;
}

int mirt_ctx_set_spheres(MirtContext* c, const MirtSphere* spheres, uint32_t n_spheres) { return set_spheres(c, spheres, n_spheres, false); }

int mirt_ctx_set_spheres_device(MirtContext* c, const void* d_spheres, uint32_t n_spheres) { return set_spheres(c, d_spheres, n_spheres, true); }

int mirt_ctx_set_camera(MirtContext* c, const MirtGpuCamera* cam)
{
    if (!c || !cam) return fail(MIRT_ERR_NULL_POINTER, "ctx/camera is null");
    if (!c->have_scene) return fail(MIRT_ERR_NO_SCENE, "set_scene has not been called");
    // No device work at all: the camera is a kernel argument of every launch (RenderArgs.cam).  Launches already
    // queued keep the camera they were issued with; the next render call uses this one.  The reference updates the
    // camera every interactive frame (layer.rs:188-193, mod.rs:353-388), so this must cost nothing.
    c->cam = *cam;
    return MIRT_OK;
}

static int check_params(const MirtContext* c, const MirtParams* p)
{
    if (!c || !p) return fail(MIRT_ERR_NULL_POINTER, "ctx/params is null");
    if (!c->have_scene) return fail(MIRT_ERR_NO_SCENE, "set_scene has not been called");
    if (p->width == 0 || p->height == 0)
        return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", p->width, p->height);
    if (p->spp == 0) return fail(MIRT_ERR_SPP_ZERO, "spp is zero");
    // the kernels count a unit's work items (up to 64 pixels x spp) and the samples of a pixel in 32 bits
    if (p->spp > MIRT_MAX_SPP_PER_CALL || (uint64_t)p->sample_begin + p->spp > 0xffffffffull)
        return fail(MIRT_ERR_SPP_RANGE, "spp %u (from sample %u) is out of range: at most %u samples per pixel in one call, sample indices below 2^32",
                    p->spp, p->sample_begin, (unsigned)MIRT_MAX_SPP_PER_CALL);
    if (p->mode != MIRT_MODE_PARITY && p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "unknown mode %u", p->mode);
    uint32_t rb, re;
    if (!rows_valid(p, &rb, &re)) return fail(MIRT_ERR_BAD_ROWS, "invalid row selection [%u,%u) of %u, part %u/%u", p->row_begin, p->row_end, p->height, p->part, p->n_parts);
    if (p->mode == MIRT_MODE_PT && p->frame_spp != 0 && (p->spp % p->frame_spp != 0 || p->sample_begin % p->frame_spp != 0))
        return fail(MIRT_ERR_FRAME_SPP, "frame_spp %u must divide spp %u and sample_begin %u", p->frame_spp, p->spp, p->sample_begin);
    if (p->mode == MIRT_MODE_PARITY) {
        if (c->parity_scene_status != MIRT_OK)
            return fail(c->parity_scene_status, "parity mode needs material_data[2] with a valid texture (layer.rs:345-351)");
    } else {
        if (c->pt_scene_status != MIRT_OK) return fail(c->pt_scene_status, "scene tables are inconsistent: %s", mirt_status_string(c->pt_scene_status));
        if ((p->flags & MIRT_FLAG_SKY_HOSEK) && !c->have_sky) return fail(MIRT_ERR_SKY, "MIRT_FLAG_SKY_HOSEK needs scene.sky");
    }
    if ((uint64_t)out_rows(p) * p->width > 0xffffffffull) return fail(MIRT_ERR_BAD_ROWS, "more than 2^32 pixels in one call");
    return MIRT_OK;
}

// ---- the ring of launch slots ----
// Wait for the launch recorded in slot i (if any) and add its kernel time to ms_folded.
static int fold_slot(MirtContext* c, size_t i)
{
    if (!c->slot_busy[i]) return MIRT_OK;
    HIP_TRY(hipEventSynchronize(c->ev_end[i]));
    float ms = 0.0f;
    if (c->slot_timed[i]) HIP_TRY(hipEventElapsedTime(&ms, c->ev_begin[i], c->ev_end[i]));    // (untimed launches carry an end event only)
    c->ms_folded += ms;
    c->launches_folded += 1;
    c->last_ms = ms;
    c->slot_busy[i] = 0;
    c->ev_in_flight -= 1;
    return MIRT_OK;
}

// Wait until a re-zeroing queued for slot i has landed.
static int await_zero(MirtContext* c, size_t i)
{
    if (!c->slot_zeroing[i]) return MIRT_OK;
    HIP_TRY(hipEventSynchronize(c->ev_zeroed[c->slot_zero_event[i]]));
    c->slot_zeroing[i] = 0;
    return MIRT_OK;
}

// Retire slots [first, first + n): fold their launches' times and -- if any of their kernels took units from the dispenser
// (slot_dirty) -- re-zero the dispenser words of all of them with ONE memset on the context's zero_stream (the eight words of a slot
// sit 4 KB apart: 32 KB per slot).  The host has seen every kernel's end before it queues the memset, so no stream ever waits on
// another stream's event; ev_zeroed[first] says when the memset has landed (await_zero).
static int retire_slots(MirtContext* c, size_t first, size_t n)
{
    bool dirty = false;
    for (size_t i = first; i < first + n; ++i) {
        int rc = await_zero(c, i);                                  // (an earlier memset of this slot: let it land first)
        if (rc == MIRT_OK) rc = fold_slot(c, i);
        if (rc != MIRT_OK) return rc;
        dirty = dirty || c->slot_dirty[i];
    }
    if (!dirty) return MIRT_OK;
    HIP_TRY(hipMemsetAsync(c->d_work_counter + first * kDispenserWords, 0, sizeof(uint32_t) * kDispenserWords * n, c->zero_stream));
    HIP_TRY(hipEventRecord(c->ev_zeroed[first], c->zero_stream));
    for (size_t i = first; i < first + n; ++i) {
        c->slot_dirty[i] = 0;
        c->slot_zeroing[i] = 1;
        c->slot_zero_event[i] = (unsigned char)first;
    }
    return MIRT_OK;
}

// The ring retires its slots in batches of 16, half a ring ahead of the slot in use (launch_render): one small fill kernel per 16
// launches instead of one per launch (per-launch fills cost the dispensed 4-spp frame 2.4 %, profiles/r04_ring_ab.txt).
constexpr size_t kRingBatch = 16;

// The blocking path (mirt_ctx_get_stats): fold every launch in flight, oldest first (last_ms = the newest launch's time), and leave
// every slot clean.
static int fold_events(MirtContext* c)
{
    const size_t n = c->ev_begin.size();
    for (size_t k = c->ev_in_flight; k > 0; --k) {
        const int rc = fold_slot(c, (c->ev_next + n - k) % n);
        if (rc != MIRT_OK) return rc;
    }
    for (size_t b = 0; b < n / kRingBatch; ++b) {
        const int rc = retire_slots(c, b * kRingBatch, kRingBatch);
        if (rc != MIRT_OK) return rc;
    }
    for (size_t i = 0; i < n; ++i) {
        const int rc = await_zero(c, i);
        if (rc != MIRT_OK) return rc;
    }
    return MIRT_OK;
}

// A launch went wrong after its kernel was enqueued: make the slot safe to reuse whatever state the stream is in.
static void poison_slot(MirtContext* c, size_t i, hipStream_t stream)
{
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(c->zero_stream);
    (void)hipMemset(c->d_work_counter + i * kDispenserWords, 0, sizeof(uint32_t) * kDispenserWords);
    if (c->slot_busy[i]) { c->slot_busy[i] = 0; c->ev_in_flight -= 1; }
    c->slot_zeroing[i] = 0;
    c->slot_dirty[i] = 0;
}

// The tree of a MIRT_SCENE_HBM scene as nearest_hit_bvh reads it from a launch's kernel arguments: one function for the render launches and
// the ray queries (launch_trace).  stack_entries: node references per lane of the launch's traversal stacks (0: MIRT_BVH_MAX_DEPTH, the strip kernels).
static void fill_bvh_args(const MirtContext* c, mirt::RenderArgs* a, uint32_t stack_entries)
{
    a->bvh_nodes = reinterpret_cast<const float4*>(c->d_bvh);
    a->bvh_recs = reinterpret_cast<const float4*>(c->d_bvh + c->bvh_off_recs);
    a->bvh_ids = reinterpret_cast<const uint32_t*>(c->d_bvh + c->bvh_off_ids);
    a->bvh_root = c->bvh_root;
    a->bvh_n_always = c->bvh_n_always;
    for (int k = 0; k < 3; ++k) a->bvh_centre[k] = c->bvh_centre[k];
    a->bvh_radius = c->bvh_radius;
    a->bvh_rmax = c->bvh_rmax;
    a->bvh_stack_entries = stack_entries;
}

// The kernel arguments a query plan decides (mirt_launch_plan.h: QueryPlan) and what of the context goes with them -- the tree, the grid,
// sph3 --, behind fill_common_args: the counterpart of fill_render_args for the query launches.
static void fill_query_args(const MirtContext* c, const mirt::QueryPlan& pl, mirt::RenderArgs* a)
{
    const bool lds_scene = mirt::query_family_lds(pl.family);
    if (!lds_scene) fill_bvh_args(c, a, pl.bvh_stack_entries);
    else for (int k = 0; k < 12; ++k) a->sph3[k] = c->sph3[k];
    if (pl.grid) { a->grid = c->d_grid; a->grid_bytes = c->grid_bytes; a->grid_flat_y = c->grid_flat_y ? 1u : 0u; }
    if (pl.rays_as_row) { a->width = pl.n_rays; a->height = 1u; }
    a->lds_bytes = pl.lds_bytes; a->n_units = pl.n_units; a->px_groups_log2 = pl.px_groups_log2;
}

// jenkins-folds a caller's 64-bit seed into the 32-bit key of a launch's RNG streams (RenderArgs.seed_mix)
static uint32_t seed_mix(uint64_t seed) { return jenkins_hash((uint32_t)seed ^ jenkins_hash((uint32_t)(seed >> 32))); }

// What every launch copies from the context and its params: the tables and counts, the sampling and row fields, seed_mix and -- unless
// `pinhole` < 0: a launch without a camera (ray queries) -- the camera.
// The kernels' pinhole shortcut (generate_primary): the flag `pinhole` travels in the padding word beside lower_left_corner of
// THIS launch's by-value copy of the camera; the caller's struct is never touched.
static void fill_common_args(const MirtContext* c, mirt::RenderArgs* a, const MirtParams& p, uint32_t rows, int pinhole)
{
    if (pinhole >= 0) {
        a->cam = c->cam;
        const uint32_t flag = (uint32_t)pinhole;
        std::memcpy(&a->cam._padding5, &flag, 4);
    }
    a->spheres = c->d_spheres; a->mats = c->d_mats; a->pmats = c->d_pmats; a->texels = c->d_texels; a->sky = c->d_sky;
    a->n_texels = c->n_texels; a->n_spheres = c->n_spheres; a->n_mats = c->n_mats;
    a->width = p.width; a->height = p.height; a->spp = p.spp; a->num_bounces = p.num_bounces; a->flags = p.flags;
    a->seed_mix = seed_mix(p.seed);
    a->sample_begin = p.sample_begin;
    a->row_begin = p.row_begin; a->tile_rows = p.tile_rows; a->n_parts = p.n_parts; a->part = p.part;
    a->out_rows = rows;
}

// the pinhole word of the launches beside launch_render (all path-traced): MIRT_PINHOLE=0 switches the shortcut off
static int pinhole_word(const MirtContext* c) { return (c->tuning.pinhole != 0 && camera_is_pinhole(c->cam)) ? 1 : 0; }

// what the launch plan reads of a context (mirt_launch_plan.h)
static mirt::PlanFacts plan_facts(const MirtContext* c)
{
    mirt::PlanFacts f{};
    f.cu_count = (uint32_t)c->cu_count; f.lds_per_cu = c->lds_per_cu; f.lds_per_block = c->lds_per_block;
    f.n_spheres = c->n_spheres; f.n_mats = c->n_mats; f.n_shading_routines = c->n_shading_routines;
    f.has_image_texture = c->has_image_texture; f.have_sky = c->have_sky; f.fits_flat = c->fits_flat; f.hbm = c->hbm;
    f.grid_bytes = c->grid_bytes; f.grid_packable = c->grid_packable; f.grid_flat_y = c->grid_flat_y; f.have_shade = c->have_shade;
    f.bvh_max_depth = c->bvh_plan.max_depth;
    f.camera_is_pinhole = camera_is_pinhole(c->cam);
    return f;
}

// The path-traced kernels exist in two builds: the bit-exact one and the opt-in fast-math one (counting launches and parity mode always
// run the exact build).  A plan picks its build HERE (kRenderKernel[plan.fast]) and nowhere else.
static mirt::RenderKernel (*const kRenderKernel[2])(const mirt::RenderPlan&) = { kx::render_kernel, kf::render_kernel };

// threads per block of the plan's launch
static uint32_t plan_threads(const mirt::RenderPlan& pl)
{
    if (pl.kernel == mirt::kKernelPtPool || pl.kernel == mirt::kKernelPtPoolHbm) return pl.pool.threads;
    return pl.launch_threads ? pl.launch_threads : mirt::kBlockThreads;
}

// Blocks of the plan's kernel that are resident per CU at once (registers and LDS decide).
static uint32_t plan_resident_per_cu(const mirt::RenderPlan& pl)
{
    if (pl.kernel == mirt::kKernelPtPool) return 0u;       // the flat and grid pool kernels: LDS alone decides (plan_render), the runtime is not asked
    const mirt::RenderKernel k = kRenderKernel[pl.fast](pl);
    // no such build (the dispatch will refuse the launch): pooled HBM has always answered "no answer", the other families one block
    if (!k) return pl.kernel == mirt::kKernelPtPoolHbm ? 0u : 1u;
    // The parity and strip kernels are asked about kBlockThreads even where the launch runs launch_threads; the HBM kernels about the
    // launch's threads.  Either number decides block counts on the device, so both stay as they were measured.
    const bool block_threads = pl.kernel == mirt::kKernelParity || pl.kernel == mirt::kKernelPtStrip;
    return kx::blocks_per_cu(k, block_threads ? mirt::kBlockThreads : plan_threads(pl), pl.lds_bytes);
}

static hipError_t dispatch_plan(const mirt::RenderPlan& pl, const mirt::RenderArgs& a, mirt::LaunchOn on)
{
    const mirt::RenderKernel k = kRenderKernel[pl.fast](pl);
    return k ? kx::launch_with_lds(k, pl.blocks, plan_threads(pl), a, on) : hipErrorInvalidValue;
}

// The ring's next slot.  When the ring enters a batch of 16 slots, the batch HALF A RING AHEAD is retired (retire_slots): its launches
// -- 32 to 17 launches old -- have normally finished long ago (the waits return at once; a caller more than 17 launches ahead of the
// GPU is held here, which is what a bounded queue should do), their times are folded and their dispenser words re-zeroed on the
// context's own stream.  By the time the ring reaches those slots they are clean: the pipeline is never drained.
static int acquire_slot(MirtContext* c, size_t ev)
{
    static_assert(kEventPool % (2 * kRingBatch) == 0, "the ring is a whole number of batch pairs");
    int rc = MIRT_OK;
    if (ev % kRingBatch == 0) rc = retire_slots(c, (ev + kEventPool / 2) % kEventPool, kRingBatch);
    if (rc == MIRT_OK && (c->slot_busy[ev] || c->slot_dirty[ev])) rc = retire_slots(c, ev, 1);   // (not in the normal flow: the batch ahead was retired 32 launches ago)
    if (rc == MIRT_OK) rc = await_zero(c, ev);               // at most one wait for the batch's memset, 32 launches old
    if (rc != MIRT_OK) return rc;
    if (c->tuning.debug_slots) {                 // MIRT_DEBUG_SLOTS=1 (tests): the slot's eight dispenser words ARE zero now
        uint32_t wds[8];
        HIP_TRY(hipMemcpy2D(wds, sizeof(uint32_t), c->d_work_counter + ev * kDispenserWords, sizeof(uint32_t) * kDispenserStride, sizeof(uint32_t), 8, hipMemcpyDeviceToHost));
        for (int k = 0; k < 8; ++k)
            if (wds[k] != 0u) return fail(MIRT_ERR_HIP, "launch slot %zu: dispenser word %d holds %u before the launch", ev, k, wds[k]);
    }
    return MIRT_OK;
}

// The kernel arguments of a planned render launch in slot `ev`: the context's tables, the caller's params and buffers, the plan's schedule.
static void fill_render_args(const MirtContext* c, const mirt::RenderPlan& pl, const MirtParams* p, uint32_t* d_out, unsigned long long* d_accum, size_t ev,
                             mirt::RenderArgs* a)
{
    const bool pt = p->mode == MIRT_MODE_PT;
    fill_common_args(c, a, *p, pl.out_rows, (int)pl.pinhole);
    a->out = d_out; a->counters = c->d_counters + ev * mirt::kNumCounters; a->work_counter = c->d_work_counter + ev * kDispenserWords; a->accum = d_accum;
    a->frame_spp = pt ? p->frame_spp : 0u;
    a->frame_begin = pt ? p->frame_begin : 0u;
    for (int q = 0; q < 5; ++q) a->queue_routine[q] = c->queue_routine[q];
    for (int k = 0; k < 12; ++k) a->sph3[k] = c->sph3[k];
    a->n_units = pl.n_units;
    for (uint32_t l = 0; l <= mirt::kStripLevels; ++l) { a->lvl_unit[l] = pl.lvl_unit[l]; a->lvl_pix[l] = pl.lvl_pix[l]; }
    a->grid = pl.use_grid ? c->d_grid : nullptr;
    a->grid_bytes = pl.use_grid ? c->grid_bytes : 0u;
    a->shade = (pl.use_grid && c->have_shade) ? c->d_shade : nullptr;
    a->grid_pool_slots = pl.grid_pool_slots; a->strip_cand = pl.strip_cand; a->grid_flat_y = pl.grid_flat_y;
    a->lds_bytes = pl.lds_bytes; a->launch_threads = pl.launch_threads;
    if (c->hbm) fill_bvh_args(c, a, pl.bvh_stack_entries);
    a->static_units = pl.static_units; a->px_groups_log2 = pl.px_groups_log2; a->stream_samples = pl.stream_samples; a->spread_units = pl.spread_units;
    a->first_dispensed = pl.first_dispensed;
    for (uint32_t x = 0; x < 8u; ++x) a->disp_taken[x] = pl.disp_taken[x];
}

// A render launch: a slot of the launch ring, the launch plan (mirt_launch_plan.h: which kernel, which geometry, which schedule), the
// kernel's occupancy, the plan's block count, the kernel arguments, one dispatch, and the slot's and the accumulation's bookkeeping.
// d_out and d_accum both set: a progressive frame (mirt_ctx_accum_frame_device): sums AND image -> the *_frame_kernel build of
// whatever schedule the plan chooses.
static int launch_render(MirtContext* c, const MirtParams* p, uint32_t* d_out, hipStream_t stream,
                         unsigned long long* d_accum = nullptr)
{
    const size_t ev = c->ev_next;
    const int rc = acquire_slot(c, ev);
    if (rc != MIRT_OK) return rc;
    mirt::RenderPlan pl = mirt::plan_render(plan_facts(c), c->tuning, *p, d_out != nullptr && d_accum != nullptr);
    if (pl.status != MIRT_OK) return fail(pl.status, "%s", pl.message);
    mirt::plan_blocks(pl, plan_resident_per_cu(pl));
    mirt::RenderArgs a{};
    fill_render_args(c, pl, p, d_out, d_accum, ev, &a);
    const bool count = pl.count;
#ifdef MIRT_DIAG_STAMPS
    HIP_TRY(hipMemsetAsync(a.counters, 0, sizeof(unsigned long long) * mirt::kNumCounters, stream));
#endif
    if (count) HIP_TRY(hipMemsetAsync(a.counters, 0, sizeof(unsigned long long) * mirt::kNumCounters, stream));
    // Events.  A TIMED launch (mirt_ctx_set_timing, the default) carries a start and an end event for mirt_ctx_get_stats; they ride on
    // the kernel dispatch itself (hipExtLaunchKernel), not as two record packets in the stream: per launch of the reference's own loop
    // (parity mode, 2 spp, 800x600) 20.6 us with records, 17.9 with the events on the dispatch, 12.9 with none (profiles/r04_ring_ab.txt
    // block 3).  An UNTIMED launch carries an end event only if something must learn that it has finished: its dispenser words have to
    // be re-zeroed (dispensed units), or its counters will be read (counting launch).  The reference's interactive frames -- units
    // dealt round-robin -- carry none.
    const bool timed = c->timing;
    const bool need_end = timed || count || a.static_units == 0u;
    const bool ext_events = c->tuning.ext_events && need_end;
    if (timed && !ext_events) HIP_TRY(hipEventRecord(c->ev_begin[ev], stream));
    const mirt::LaunchOn on = ext_events ? mirt::LaunchOn(stream, timed ? c->ev_begin[ev] : nullptr, c->ev_end[ev]) : mirt::LaunchOn(stream);
    HIP_TRY(dispatch_plan(pl, a, on));
    mirt::plan_kernel_name(pl, c->last_kernel, sizeof c->last_kernel);
    // The kernel is enqueued: from here on the slot is in use, whatever happens below (a failure after this point must not hand the
    // slot -- its dispenser words no longer zero -- to the next launch: poison_slot).
    c->ev_next = (ev + 1) % c->ev_begin.size();
    hipError_t he = hipSuccess;
    if (need_end) {
        c->slot_busy[ev] = 1;
        c->slot_timed[ev] = timed ? 1 : 0;
        c->ev_in_flight += 1;
        if (!ext_events) he = hipEventRecord(c->ev_end[ev], stream);
    } else {                                      // nothing will ever wait for this launch through the context ...
        c->launches_folded += 1;
        c->last_ms = 0.0;
        if (stream != c->stream && std::find(c->untimed_streams.begin(), c->untimed_streams.end(), stream) == c->untimed_streams.end())
            c->untimed_streams.push_back(stream);   // ... except mirt_ctx_synchronize / _destroy, through its stream
    }
    // Kernels that take units from the dispenser leave its words non-zero: retire_slots re-zeroes them before the slot's next use, on the
    // context's zero_stream -- never a memset node on the caller's stream, where it costs 3 us between kernels.  Launches whose units are
    // dealt round-robin (the reference's 2-spp frames, parity mode's lane = pixel) never touch the words.
    if (a.static_units == 0u) c->slot_dirty[ev] = 1;
    if (d_accum) c->accum_stream = stream;
    if (he == hipSuccess && d_accum && stream != c->stream) {   // resolve/read (on the context's stream) must see sums added on a caller stream
        he = hipEventRecord(c->ev_accum, stream);
        if (he == hipSuccess) c->accum_pending = true;
    }
    if (he != hipSuccess) {
        poison_slot(c, ev, stream);
        return fail(MIRT_ERR_HIP, "%s", hipGetErrorString(he));
    }
    c->last_slot = ev;
    c->stats_counted = count;
    c->stats = MirtStats{};
    c->stats.samples = (uint64_t)pl.out_rows * p->width * p->spp;
    return MIRT_OK;
}

int mirt_ctx_render_device(MirtContext* c, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream)
{
    int rc = check_params(c, p);
    if (rc != MIRT_OK) return rc;
    if (!d_out) return fail(MIRT_ERR_NULL_POINTER, "d_out_rgba8 is null");
    const size_t need = (size_t)out_rows(p) * p->width * 4;
    if (out_len < need) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %zu needed", out_len, need);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    return launch_render(c, p, (uint32_t*)d_out, st);
}

int mirt_ctx_render(MirtContext* c, const MirtParams* p, uint8_t* out, size_t out_len)
{
    int rc = check_params(c, p);
    if (rc != MIRT_OK) return rc;
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out_rgba8 is null");
    const size_t npix = (size_t)out_rows(p) * p->width;
    if (out_len < npix * 4) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %zu needed", out_len, npix * 4);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_capacity(&c->d_out, &c->cap_out, npix)) != MIRT_OK) return rc;
    if ((rc = launch_render(c, p, c->d_out, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_out, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

const char* mirt_ctx_last_kernel(const MirtContext* c) { return c ? c->last_kernel : ""; }

int mirt_ctx_synchronize(MirtContext* c)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    HIP_TRY(hipSetDevice(c->device));
    for (size_t i = 0; i < c->ev_begin.size(); ++i) if (c->slot_busy[i]) HIP_TRY(hipEventSynchronize(c->ev_end[i]));
    HIP_TRY(hipStreamSynchronize(c->zero_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->frame_stream_b) HIP_TRY(hipStreamSynchronize(c->frame_stream_b));
    for (hipStream_t st : c->untimed_streams) HIP_TRY(hipStreamSynchronize(st));      // launches that carried no event (mirt_ctx_set_timing(0))
    c->untimed_streams.clear();
    if (c->trace_pending) HIP_TRY(hipEventSynchronize(c->ev_trace_end));              // a ray query on a caller stream (mirt_ctx_trace_stats folds it)
    if (c->adapt_pending) HIP_TRY(hipEventSynchronize(c->ev_adapt_end));              // an adaptive step on a caller stream (mirt_ctx_adapt_stats folds it)
    return MIRT_OK;
}

// Two streams of the context for hosts that keep two frames in flight.  Stream 0 is the context's own stream (normal priority); stream 1 is
// created here, on first use, with the device's HIGHEST priority: HIP keeps its hardware queues per priority, so the two can never share
// one -- two normal-priority streams share a queue whenever the process holds more streams than the runtime has queues (4 by default),
// and kernels of streams on one queue run strictly one after the other (measured with torch's pool streams: 1080p, 2 spp: 98.6 us per
// frame on a shared queue, 77.8 on two queues, 83.4 for this pair; profiles/r04_ring_ab.txt block 7).
int mirt_ctx_frame_stream(MirtContext* c, uint32_t index, void** out_hip_stream)
{
    if (!c || !out_hip_stream) return fail(MIRT_ERR_NULL_POINTER, "ctx/out_hip_stream is null");
    if (index > 1u) return fail(MIRT_ERR_BAD_ROWS, "a context has frame streams 0 and 1, not %u", index);
    HIP_TRY(hipSetDevice(c->device));
    if (index == 1u && !c->frame_stream_b) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&c->frame_stream_b, hipStreamNonBlocking, greatest));
    }
    *out_hip_stream = index == 0u ? (void*)c->stream : (void*)c->frame_stream_b;
    return MIRT_OK;
}

int mirt_ctx_set_timing(MirtContext* c, int enabled)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    c->timing = enabled != 0;
    return MIRT_OK;
}

int mirt_ctx_get_stats(MirtContext* c, MirtStats* out)
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    HIP_TRY(hipSetDevice(c->device));
    const bool had_launch = c->ev_in_flight > 0 || c->launches_folded > 0;
    const int rc = fold_events(c);
    if (rc != MIRT_OK) return rc;
    c->stats.kernel_ms = c->last_ms;
    c->stats.kernel_ms_total = c->ms_folded;
    c->stats.launches = c->launches_folded;
    c->ms_folded = 0.0;
    c->launches_folded = 0;
#ifdef MIRT_DIAG_STAMPS
    if (had_launch) {                            // wave-cycles per section of the pooled kernel (mirt_kernels.hip: Stamps)
        unsigned long long h[mirt::kNumCounters];
        HIP_TRY(hipMemcpy(h, c->d_counters + c->last_slot * mirt::kNumCounters, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "MIRT_STAMPS pop %llu gen %llu scatter %llu big %llu setup_fresh %llu cells_fresh %llu tail %llu setup_resume %llu cells_resume %llu strip_end %llu\n",
                h[18], h[19], h[20], h[21], h[22], h[23], h[24], h[25], h[26], h[27]);
    }
#endif
    if (had_launch && c->stats_counted) {
        unsigned long long h[mirt::kNumCounters];
        HIP_TRY(hipMemcpy(h, c->d_counters + c->last_slot * mirt::kNumCounters, sizeof h, hipMemcpyDeviceToHost));
        c->stats.rays = h[mirt::kCntRays];
        c->stats.sphere_tests = h[mirt::kCntTests];
        c->stats.roots = h[mirt::kCntRoots];
        c->stats.hits = h[mirt::kCntHits];
        for (int i = 0; i < 5; ++i) c->stats.scatter[i] = h[mirt::kCntScatter0 + i];

        c->stats.sky_misses = h[mirt::kCntSky];
        c->stats.lane_iterations = h[mirt::kCntLaneIters];
        c->stats.wave_iterations = h[mirt::kCntWaveIters];
        c->stats.grid_cells = h[mirt::kCntCells];
        c->stats.grid_wave_cells = h[mirt::kCntWaveCells];
        c->stats.texel_fetches[0] = h[mirt::kCntTexelsPrimary];
        c->stats.texel_fetches[1] = h[mirt::kCntTexelsLater];
        c->stats.texel_tile_hits[0] = h[mirt::kCntTileHitsPrimary];
        c->stats.texel_tile_hits[1] = h[mirt::kCntTileHitsLater];
#ifdef MIRT_DIAG_STEPS
        fprintf(stderr, "MIRT_DIAG steps scatter/gen/walk %llu %llu %llu paths %llu %llu %llu ff_steps %llu traces cut/hit/miss %llu %llu %llu strips %llu with_list %llu candidates %llu\n",
                h[18], h[19], h[20], h[21], h[22], h[23], h[24], h[25], h[26], h[27], h[28], h[29], h[30]);
#endif
#ifdef MIRT_PROBE_TEXELS
        c->stats.grid_cells = h[12]; c->stats.grid_wave_cells = h[13]; c->stats.lane_iterations = h[14]; c->stats.wave_iterations = h[15];
#endif
#ifdef MIRT_PROBE_UNIFORM_NEXT
        c->stats.grid_cells = h[14]; c->stats.grid_wave_cells = h[15]; c->stats.scatter[4] = h[12]; c->stats.roots = h[13];
#endif
        c->stats_counted = false;
    }
    *out = c->stats;
    return MIRT_OK;
}

// ---- ray queries against the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
// What both entry points check, in the header's order; MIRT_OK with *go = false: nothing to do (n_rays == 0).
static int check_trace(const MirtContext* c, const void* rays, uint32_t n, uint32_t flags, const void* hits, bool* go)
{
    *go = false;
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    if (flags & ~(uint32_t)(MIRT_RAYS_FLAT | MIRT_RAYS_ANY_HIT | MIRT_RAYS_COUNT | MIRT_RAYS_SORT | MIRT_QUERY_LDS)) return fail(MIRT_ERR_BAD_MODE, "unknown MIRT_RAYS_* bits 0x%x", flags);
    if (n && (!rays || !hits)) return fail(MIRT_ERR_NULL_POINTER, "rays/hits is null");
    if (!c->have_scene || (!c->hbm && !(flags & MIRT_QUERY_LDS))) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene (a scene in LDS takes MIRT_QUERY_LDS)");
    if (!c->hbm) {                                           // MIRT_QUERY_LDS on a scene in LDS: the layout, last
        const mirt::QueryPlan pl = mirt::plan_trace(plan_facts(c), c->tuning, n, flags);
        if (pl.status != MIRT_OK) return fail(pl.status, "%s", pl.message);
    }
    *go = n != 0u;
    return MIRT_OK;
}

// MIRT_RAYS_SORT / MIRT_RADIANCE_SORT: queue the codes of n > 0 rays and their sort on `st` (after the caller has recorded the begin event, so
// that kernel_ms spans them); *d_order = the permutation for the query kernel that follows on the same stream.  No host synchronisation
// unless the context's scratch must grow.  The bounds are the resident tree's, those of mirt_ctx_bvh_info.
static int queue_ray_sort(MirtContext* c, const void* d_rays, uint32_t n, hipStream_t st, const uint32_t** d_order)
{
    const int rc = mirt::ray_sort_order(d_rays, n, c->bvh_centre, c->bvh_radius, st, &c->ray_sort, &c->ray_sort_off_order);
    if (rc != MIRT_OK) return rc;
    c->ray_sort_n = n;
    c->ray_sort_any = true;
    *d_order = reinterpret_cast<const uint32_t*>(c->ray_sort.d + c->ray_sort_off_order);
    return MIRT_OK;
}

// The tail of a ray query, a feature frame and a radiance query: the plan's kernel on `st` behind ev_trace_begin, its name, ev_trace_end, and
// what mirt_ctx_trace_stats will wait for and fold.
static int queue_query(MirtContext* c, const mirt::QueryPlan& pl, const mirt::RenderArgs& a, const mirt::QueryBuffers& b, hipStream_t st, bool timed)
{
    HIP_TRY(kx::launch_query(pl, a, b, st));
    mirt::query_kernel_name(pl, c->last_kernel, sizeof c->last_kernel);
    HIP_TRY(hipEventRecord(c->ev_trace_end, st));
    c->trace_pending = true;
    c->trace_timed = timed;
    c->trace_counted = pl.count;
    c->trace_stats = MirtRayStats{};
    return MIRT_OK;
}

// An MIRT_QUERY_LDS launch runs a persistent grid: its kernel's occupancy bounds the blocks, as an MIRT_ADAPT_LDS step's does (queue_adapt_steps)
static void size_query_grid(mirt::QueryPlan& pl)
{
    if (mirt::query_family_lds(pl.family)) mirt::query_plan_blocks(pl, kx::blocks_per_cu(kx::query_kernel(pl), pl.threads, pl.lds_bytes));
}

// Queue trace_rays_kernel<bvh, any, count> (trace_rays_sorted_kernel behind the code kernel and the sort with MIRT_RAYS_SORT) for n > 0 rays in
// device memory on `st`.  No host synchronisation.
static int launch_trace(MirtContext* c, const void* d_rays, uint32_t n, uint32_t flags, void* d_hits, hipStream_t st)
{
    mirt::QueryPlan pl = mirt::plan_trace(plan_facts(c), c->tuning, n, flags);
    size_query_grid(pl);
    mirt::RenderArgs a{};
    fill_common_args(c, &a, MirtParams{}, 0u, -1);
    a.counters = c->d_trace_counters;
    fill_query_args(c, pl, &a);
    const bool timed = c->timing;
    mirt::QueryBuffers b{ d_rays, d_hits, nullptr, nullptr };
    if (pl.sorted) {      // first: a failed allocation leaves nothing queued
        if (timed) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
        const int rc = queue_ray_sort(c, d_rays, n, st, &b.order);
        if (rc != MIRT_OK) return rc;
    }
    if (pl.count) HIP_TRY(hipMemsetAsync(c->d_trace_counters, 0, sizeof(unsigned long long) * mirt::kNumCounters, st));
    if (timed && !pl.sorted) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
    return queue_query(c, pl, a, b, st, timed);
}

int mirt_ctx_trace_rays_device(MirtContext* c, const void* d_rays, uint32_t n_rays, uint32_t flags, void* d_hits, void* hip_stream)
{
    bool go;
    const int rc = check_trace(c, d_rays, n_rays, flags, d_hits, &go);
    if (rc != MIRT_OK || !go) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_trace(c, d_rays, n_rays, flags, d_hits, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_trace_rays(MirtContext* c, const MirtRay* rays, uint32_t n_rays, uint32_t flags, MirtRayHit* hits)
{
    bool go;
    int rc = check_trace(c, rays, n_rays, flags, hits, &go);
    if (rc != MIRT_OK || !go) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)n_rays * sizeof(MirtRay);
    static_assert(sizeof(MirtRay) == sizeof(MirtRayHit), "one size for both staging buffers");
    if ((rc = ensure_capacity(&c->d_trace_rays, &c->cap_trace_rays, bytes)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_trace_hits, &c->cap_trace_hits, bytes)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_trace_rays, rays, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_trace(c, c->d_trace_rays, n_rays, flags, c->d_trace_hits, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hits, c->d_trace_hits, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_ray_sort_code(const float centre[3], float radius, const void* ray32, uint32_t* out_code)
{
    if (!centre || !ray32 || !out_code) return fail(MIRT_ERR_NULL_POINTER, "centre/ray/out_code is null");
    *out_code = mirt::ray_sort_code(centre, radius, ray32);
    return MIRT_OK;
}

int mirt_ctx_trace_order_read(MirtContext* c, uint32_t* order, size_t len)
{
    if (!c) return fail(MIRT_ERR_NULL_POINTER, "ctx is null");
    if (!c->ray_sort_any) return fail(MIRT_ERR_NO_SCENE, "no sorted launch has run on this context");
    if (len < c->ray_sort_n) return fail(MIRT_ERR_OUT_BUFFER, "the order holds %u indices, room for %zu", c->ray_sort_n, len);
    if (!order) return fail(MIRT_ERR_NULL_POINTER, "order is null");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());      // the sort may be in flight on a caller's stream
    HIP_TRY(hipMemcpy(order, c->ray_sort.d + c->ray_sort_off_order, sizeof(uint32_t) * (size_t)c->ray_sort_n, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

int mirt_ctx_trace_stats(MirtContext* c, MirtRayStats* out)
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    if (c->trace_pending) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev_trace_end));
        c->trace_pending = false;
        if (c->trace_timed) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_trace_begin, c->ev_trace_end));
            c->trace_stats.kernel_ms = ms;
        }
        if (c->trace_counted) {
            unsigned long long h[mirt::kNumCounters];
            HIP_TRY(hipMemcpy(h, c->d_trace_counters, sizeof h, hipMemcpyDeviceToHost));
            c->trace_stats.rays = h[mirt::kCntRays];
            c->trace_stats.sphere_tests = h[mirt::kCntTests];
            c->trace_stats.roots = h[mirt::kCntRoots];
            c->trace_stats.hits = h[mirt::kCntHits];
            c->trace_stats.nodes = h[mirt::kCntCells];
            c->trace_stats.wave_nodes = h[mirt::kCntWaveCells];
        }
    }
    *out = c->trace_stats;
    return MIRT_OK;
}

// ---- first-hit feature frames of the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
// What both entry points check, in the header's order.  Nothing is queued before the last of them has passed.
static int check_features(const MirtContext* c, const MirtParams* p, uint32_t flags, const void* out, size_t out_len)
{
    if (!c || !p || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/out is null");
    if (flags & ~(uint32_t)(MIRT_FEATURES_FLAT | MIRT_QUERY_LDS)) return fail(MIRT_ERR_BAD_MODE, "unknown MIRT_FEATURES_* bits 0x%x", flags);
    if (!c->have_scene || (!c->hbm && !(flags & MIRT_QUERY_LDS))) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene (a scene in LDS takes MIRT_QUERY_LDS)");
    if (p->width == 0 || p->height == 0)
        return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", p->width, p->height);
    uint32_t rb, re;
    if (!rows_valid(p, &rb, &re)) return fail(MIRT_ERR_BAD_ROWS, "invalid row selection [%u,%u) of %u, part %u/%u", p->row_begin, p->row_end, p->height, p->part, p->n_parts);
    if ((uint64_t)out_rows(p) * p->width > 0xffffffffull) return fail(MIRT_ERR_BAD_ROWS, "more than 2^32 pixels in one call");
    if (p->spp > MIRT_MAX_SPP_PER_CALL || (uint64_t)p->sample_begin + p->spp > 0xffffffffull)
        return fail(MIRT_ERR_SPP_RANGE, "spp %u (from sample %u) is out of range: at most %u samples per pixel in one call, sample indices below 2^32",
                    p->spp, p->sample_begin, (unsigned)MIRT_MAX_SPP_PER_CALL);
    if (p->frame_spp != 0) return fail(MIRT_ERR_FRAME_SPP, "frame_spp %u: a feature frame has no per-frame RNG stream, pass 0", p->frame_spp);
    const size_t need = (size_t)out_rows(p) * p->width * sizeof(MirtFeaturePixel);
    if (out_len < need) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %zu needed", out_len, need);
    if (c->pt_scene_status != MIRT_OK) return fail(c->pt_scene_status, "scene tables are inconsistent: %s", mirt_status_string(c->pt_scene_status));
    if (!c->hbm) {                                           // MIRT_QUERY_LDS on a scene in LDS: the layout, last
        const mirt::QueryPlan pl = mirt::plan_features(plan_facts(c), c->tuning, *p, flags);
        if (pl.status != MIRT_OK) return fail(pl.status, "%s", pl.message);
    }
    return MIRT_OK;
}

// Queue feature_frame_kernel<bvh> for the pixels `p` selects on `st`.  No host synchronisation.  The launch ring, MirtStats and the
// accumulation stay as they are; the event pair and the pending flag are the ray queries' (mirt_ctx_trace_stats folds the time).
static int launch_features(MirtContext* c, const MirtParams* p, uint32_t flags, void* d_out, hipStream_t st)
{
    mirt::QueryPlan pl = mirt::plan_features(plan_facts(c), c->tuning, *p, flags);
    size_query_grid(pl);
    mirt::RenderArgs a{};
    fill_common_args(c, &a, *p, out_rows(p), pinhole_word(c));     // the camera with generate_primary's pinhole word, as in launch_render
    fill_query_args(c, pl, &a);                                    // traversal stacks as for ray queries
    const bool timed = c->timing;
    if (timed) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
    return queue_query(c, pl, a, mirt::QueryBuffers{ nullptr, d_out, nullptr, nullptr }, st, timed);
}

int mirt_ctx_render_features_device(MirtContext* c, const MirtParams* p, uint32_t flags, void* d_out, size_t out_len, void* hip_stream)
{
    const int rc = check_features(c, p, flags, d_out, out_len);
    if (rc != MIRT_OK || out_rows(p) == 0u) return rc;                 // (a part of a tile partition may own no row: nothing to do)
    HIP_TRY(hipSetDevice(c->device));
    return launch_features(c, p, flags, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_render_features(MirtContext* c, const MirtParams* p, uint32_t flags, MirtFeaturePixel* out, size_t out_len)
{
    int rc = check_features(c, p, flags, out, out_len);
    if (rc != MIRT_OK || out_rows(p) == 0u) return rc;
    HIP_TRY(hipSetDevice(c->device));
    static_assert(sizeof(MirtFeaturePixel) == sizeof(MirtRayHit), "the host path stages its records where a host trace stages its hits");
    const size_t bytes = (size_t)out_rows(p) * p->width * sizeof(MirtFeaturePixel);
    if ((rc = ensure_capacity(&c->d_trace_hits, &c->cap_trace_hits, bytes)) != MIRT_OK) return rc;
    if ((rc = launch_features(c, p, flags, c->d_trace_hits, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_trace_hits, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_camera_pixel_ray(const MirtGpuCamera* cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, MirtRay* out)
{
    if (!cam || !out) return fail(MIRT_ERR_NULL_POINTER, "camera/out is null");
    if (width == 0 || height == 0) return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", width, height);
    if (x >= width || y >= height) return fail(MIRT_ERR_BAD_ROWS, "pixel (%u, %u) lies outside the %u x %u viewport", x, y, width, height);
    // feature_frame_kernel's centre ray, operation for operation (this file is compiled with -ffp-contract=off: the only fused
    // operations are the two fmaf per component)
    const float inv_w = 1.0f / (float)width, inv_h = 1.0f / (float)height;
    const float u = ((float)x + 0.5f) * inv_w;
    const float v = 1.0f - ((float)y + 0.5f) * inv_h;
    for (int k = 0; k < 3; ++k) {
        out->origin[k] = cam->eye[k];
        out->direction[k] = std::fmaf(v, cam->vertical[k], std::fmaf(u, cam->horizontal[k], cam->lower_left_corner[k])) - cam->eye[k];
    }
    out->t_max = 1000.0f;
    out->_pad = 0.0f;
    return MIRT_OK;
}

// ---- path-traced radiance for a caller's rays against the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
// What both entry points check, in the header's order; MIRT_OK with *go = false: nothing to do (n_rays == 0).
static int check_radiance(const MirtContext* c, const void* rays, uint32_t n, const MirtRadianceParams* p, const void* out, bool* go)
{
    *go = false;
    if (!c || !p) return fail(MIRT_ERR_NULL_POINTER, "ctx/params is null");
    if (n && (!rays || !out)) return fail(MIRT_ERR_NULL_POINTER, "rays/out is null");
    if (p->flags & ~(uint32_t)(MIRT_RADIANCE_FLAT | MIRT_RADIANCE_ACCUMULATE | MIRT_RADIANCE_SKY_HOSEK | MIRT_RADIANCE_SORT | MIRT_RADIANCE_POOL | MIRT_QUERY_LDS))
        return fail(MIRT_ERR_BAD_MODE, "unknown MIRT_RADIANCE_* bits 0x%x", p->flags);
    if (!c->have_scene || (!c->hbm && !(p->flags & MIRT_QUERY_LDS))) return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene (a scene in LDS takes MIRT_QUERY_LDS)");
    if (p->spp == 0) return fail(MIRT_ERR_SPP_ZERO, "spp is zero");
    if (p->spp > MIRT_MAX_SPP_PER_CALL || (uint64_t)p->sample_begin + p->spp > 0xffffffffull)
        return fail(MIRT_ERR_SPP_RANGE, "spp %u (from sample %u) is out of range: at most %u samples per ray in one call, sample indices below 2^32",
                    p->spp, p->sample_begin, (unsigned)MIRT_MAX_SPP_PER_CALL);
    if (c->pt_scene_status != MIRT_OK) return fail(c->pt_scene_status, "scene tables are inconsistent: %s", mirt_status_string(c->pt_scene_status));
    if ((p->flags & MIRT_RADIANCE_SKY_HOSEK) && !c->have_sky) return fail(MIRT_ERR_SKY, "MIRT_RADIANCE_SKY_HOSEK needs scene.sky");
    if (!c->hbm) {                                           // MIRT_QUERY_LDS on a scene in LDS: the layout, last
        const mirt::QueryPlan pl = mirt::plan_radiance(plan_facts(c), c->tuning, n, *p);
        if (pl.status != MIRT_OK) return fail(pl.status, "%s", pl.message);
    }
    *go = n != 0u;
    return MIRT_OK;
}

// Queue radiance_rays_kernel<hosek, bvh> (radiance_rays_sorted_kernel behind the code kernel and the sort with MIRT_RADIANCE_SORT) for n > 0 rays in
// device memory on `st`.  No host synchronisation.  The launch ring, MirtStats and
// the accumulation stay as they are; the event pair and the pending flag are the ray queries' (mirt_ctx_trace_stats folds the time).
// MIRT_RADIANCE_POOL on the BVH build: radiance_rays_pool_kernel in the geometry the pooled render would take for the resident tree
// (plan_bvh_pool), where the pool's own limits allow it -- 8-bit bounce counters, a geometry that fits beside the stacks of a tree this
// deep; otherwise the launch is the one without the flag.
static int launch_radiance(MirtContext* c, const void* d_rays, uint32_t n, const MirtRadianceParams* p, void* d_out, hipStream_t st)
{
    mirt::QueryPlan pl = mirt::plan_radiance(plan_facts(c), c->tuning, n, *p);
    size_query_grid(pl);
    MirtParams q{};                                       // the query's sampling fields as a render call's; no frame, no rows
    q.spp = p->spp; q.num_bounces = p->num_bounces; q.flags = p->flags; q.seed = p->seed; q.sample_begin = p->sample_begin;
    mirt::RenderArgs a{};
    fill_common_args(c, &a, q, 0u, -1);                   // (the camera stays zero: a query has none)
    fill_query_args(c, pl, &a);
    const bool timed = c->timing;
    if (timed) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
    mirt::QueryBuffers b{ d_rays, d_out, nullptr, nullptr };
    if (pl.sorted) {
        const int rc = queue_ray_sort(c, d_rays, n, st, &b.order);
        if (rc != MIRT_OK) return rc;
    }
    return queue_query(c, pl, a, b, st, timed);
}

int mirt_ctx_trace_radiance_device(MirtContext* c, const void* d_rays, uint32_t n_rays, const MirtRadianceParams* p, void* d_out, void* hip_stream)
{
    bool go;
    const int rc = check_radiance(c, d_rays, n_rays, p, d_out, &go);
    if (rc != MIRT_OK || !go) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_radiance(c, d_rays, n_rays, p, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_trace_radiance(MirtContext* c, const MirtRadianceRay* rays, uint32_t n_rays, const MirtRadianceParams* p, MirtRadiance* out)
{
    bool go;
    int rc = check_radiance(c, rays, n_rays, p, out, &go);
    if (rc != MIRT_OK || !go) return rc;
    HIP_TRY(hipSetDevice(c->device));
    static_assert(sizeof(MirtRadianceRay) == sizeof(MirtRay) && sizeof(MirtRadiance) == sizeof(MirtRayHit), "the host path stages where a host trace stages");
    const size_t bytes = (size_t)n_rays * sizeof(MirtRadianceRay);
    if ((rc = ensure_capacity(&c->d_trace_rays, &c->cap_trace_rays, bytes)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_trace_hits, &c->cap_trace_hits, bytes)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_trace_rays, rays, bytes, hipMemcpyHostToDevice, c->stream));
    if (p->flags & MIRT_RADIANCE_ACCUMULATE) HIP_TRY(hipMemcpyAsync(c->d_trace_hits, out, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_radiance(c, c->d_trace_rays, n_rays, p, c->d_trace_hits, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_trace_hits, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_ctx_accum_reset(MirtContext* c, const MirtParams* p)
{
    int rc = check_params(c, p);
    if (rc != MIRT_OK) return rc;
    if (p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "progressive accumulation exists in path-traced mode only");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t npix = (uint64_t)out_rows(p) * p->width;
    if (c->accum_pending) { HIP_TRY(hipEventSynchronize(c->ev_accum)); c->accum_pending = false; }   // no add may still be running
    if ((rc = ensure_capacity(&c->d_accum, &c->cap_accum, (size_t)npix * 3)) != MIRT_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->d_accum, 0, (size_t)npix * 3 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->accum_stream = nullptr;
    c->accum_pixels = npix;
    c->accum_samples = 0;
    c->accum_width = p->width;
    c->accum_rows = out_rows(p);
    return MIRT_OK;
}

int mirt_ctx_accum_add(MirtContext* c, const MirtParams* p, void* hip_stream)
{
    int rc = check_params(c, p);
    if (rc != MIRT_OK) return rc;
    if (p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "progressive accumulation exists in path-traced mode only");
    if (!c->d_accum || c->accum_width != p->width || c->accum_rows != out_rows(p))
        return fail(MIRT_ERR_OUT_BUFFER, "accumulation buffer does not match these params: call mirt_ctx_accum_reset first");
    HIP_TRY(hipSetDevice(c->device));
    MirtParams q = *p;
    q.sample_begin = c->accum_samples;                  // continue the RNG stream where the last frame stopped
    // check_params saw the CALLER's sample_begin; the one that counts is this one.  A caller that changes frame_spp between adds
    // without a reset would start mid-frame: the lane-per-pixel kernel seeds only at frame boundaries, so the sums would be wrong silently.
    if ((uint64_t)q.sample_begin + q.spp > 0xffffffffull)
        return fail(MIRT_ERR_SPP_RANGE, "%u samples accumulated so far + %u would pass 2^32: reset first", q.sample_begin, q.spp);
    if (q.frame_spp != 0 && q.sample_begin % q.frame_spp != 0)
        return fail(MIRT_ERR_FRAME_SPP, "frame_spp %u does not divide the %u samples accumulated so far: reset first", q.frame_spp, q.sample_begin);
    rc = launch_render(c, &q, nullptr, hip_stream ? (hipStream_t)hip_stream : c->stream, c->d_accum);
    if (rc == MIRT_OK) c->accum_samples += p->spp;
    return rc;
}

// A progressive frame reads -- and, unless spp == 0, rewrites -- the sums the previous one left: frames that alternate between streams (two
// in flight on mirt_ctx_frame_stream) are ordered here, on the device -- the new stream waits for what the stream of the LAST USER of the
// sums holds.  Every frame becomes that last user, the spp == 0 frame too: an adding frame that followed it on another stream would
// otherwise rewrite sums resolve_accum_kernel is still reading.  The frames thus form one chain, whatever streams they are on.
// hipStreamLegacy takes no part in event waits (see mirt_ctx_accum_resolve): the host waits for it instead.
static int order_frame(MirtContext* c, hipStream_t st)
{
    const hipStream_t prev = c->accum_stream;
    if (!prev || prev == st) return MIRT_OK;
    if (prev == hipStreamLegacy || st == hipStreamLegacy) {
        HIP_TRY(hipStreamSynchronize(prev));
        return MIRT_OK;
    }
    HIP_TRY(hipEventRecord(c->ev_order, prev));
    HIP_TRY(hipStreamWaitEvent(st, c->ev_order, 0));
    return MIRT_OK;
}

// What a progressive frame with these params is refused for before anything is queued, the output apart; *q = the params the launch
// runs with.  (Also behind mirt::check_accum_frame: the node asks every member before it queues a frame on any.)
static int check_frame_params(const MirtContext* c, const MirtParams* p, MirtParams* q)
{
    if (!c || !p) return fail(MIRT_ERR_NULL_POINTER, "ctx/params is null");
    *q = *p;
    if (p->spp == 0) q->spp = (p->mode == MIRT_MODE_PT && p->frame_spp) ? p->frame_spp : 1u;   // the frame after the accumulation is complete: every other field is checked as usual
    const int rc = check_params(c, q);
    if (rc != MIRT_OK) return rc;
    q->spp = p->spp;
    if (p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "progressive accumulation exists in path-traced mode only");
    if (p->spp == 0 && (!c->d_accum || c->accum_samples == 0)) return fail(MIRT_ERR_NO_SCENE, "nothing accumulated yet");
    if (!c->d_accum || c->accum_width != p->width || c->accum_rows != out_rows(p))
        return fail(MIRT_ERR_OUT_BUFFER, "accumulation buffer does not match these params: call mirt_ctx_accum_reset first");
    q->sample_begin = c->accum_samples;                 // continue the RNG stream where the last frame stopped (as mirt_ctx_accum_add)
    if (p->spp != 0) {
        if ((uint64_t)q->sample_begin + q->spp > 0xffffffffull)
            return fail(MIRT_ERR_SPP_RANGE, "%u samples accumulated so far + %u would pass 2^32: reset first", q->sample_begin, q->spp);
        if (q->frame_spp != 0 && q->sample_begin % q->frame_spp != 0)
            return fail(MIRT_ERR_FRAME_SPP, "frame_spp %u does not divide the %u samples accumulated so far: reset first", q->frame_spp, q->sample_begin);
    }
    return MIRT_OK;
}

// ... and with the output both forms write
static int check_frame(const MirtContext* c, const MirtParams* p, const void* out, size_t out_len, MirtParams* q)
{
    const int rc = check_frame_params(c, p, q);
    if (rc != MIRT_OK) return rc;
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "the output buffer is null");
    const size_t need = (size_t)c->accum_pixels * 4;
    if (out_len < need) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %zu needed", out_len, need);
    return MIRT_OK;
}

// One progressive frame into device memory on `st`: ONE launch -- the frame build of the schedule mirt_ctx_accum_add would run, or,
// once nothing is to be added (spp == 0), the resolve of what is there.  No host synchronisation.
static int launch_frame(MirtContext* c, const MirtParams* q, uint32_t* d_out, hipStream_t st)
{
    int rc = order_frame(c, st);
    if (rc != MIRT_OK) return rc;
    if (q->spp != 0) {
        rc = launch_render(c, q, d_out, st, c->d_accum);
        if (rc == MIRT_OK) c->accum_samples += q->spp;
        return rc;
    }
    // the sums are complete: the reference keeps showing their mean (mod.rs:350)
    HIP_TRY(kx::launch_resolve(c->d_accum, d_out, c->accum_pixels, c->accum_samples, q->flags, st));
    snprintf(c->last_kernel, sizeof c->last_kernel, "resolve_accum_kernel");
    c->accum_stream = st;                               // the next frame, on whatever stream, is ordered after this read (order_frame)
    if (st != c->stream) {                              // mirt_ctx_accum_reset / _resolve / _read (host waits on ev_accum) must not overtake this read.  The frames are
                                                        // one chain, so the event of the last one covers every earlier one.  (mirt_ctx_accum_add waits for nothing: an
                                                        // add after a frame on another stream is ordered by the caller, as adds among themselves are.)
        HIP_TRY(hipEventRecord(c->ev_accum, st));
        c->accum_pending = true;
        if (std::find(c->untimed_streams.begin(), c->untimed_streams.end(), st) == c->untimed_streams.end()) c->untimed_streams.push_back(st);
    }
    return MIRT_OK;
}

int mirt_ctx_accum_frame_device(MirtContext* c, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream)
{
    MirtParams q;
    const int rc = check_frame(c, p, d_out, out_len, &q);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_frame(c, &q, (uint32_t*)d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_accum_frame(MirtContext* c, const MirtParams* p, uint8_t* out, size_t out_len)
{
    MirtParams q;
    int rc = check_frame(c, p, out, out_len, &q);
    if (rc != MIRT_OK) return rc;
    const size_t npix = (size_t)c->accum_pixels;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_capacity(&c->d_out, &c->cap_out, npix)) != MIRT_OK) return rc;
    if ((rc = launch_frame(c, &q, c->d_out, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_out, npix * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

uint32_t mirt_ctx_accum_samples(const MirtContext* c) { return c ? c->accum_samples : 0u; }

int mirt_ctx_accum_resolve(MirtContext* c, const MirtParams* p, uint8_t* out, size_t out_len)
{
    if (!c || !p || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/out is null");
    if (!c->d_accum || c->accum_samples == 0) return fail(MIRT_ERR_NO_SCENE, "nothing accumulated yet");
    if (out_len < c->accum_pixels * 4) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %llu needed", out_len,
                                                    (unsigned long long)c->accum_pixels * 4);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_capacity(&c->d_out, &c->cap_out, (size_t)c->accum_pixels)) != MIRT_OK) return rc;
    // adds may sit on a caller stream: the HOST waits for the last of them (this call blocks anyway).  Never hipStreamWaitEvent here: with the
    // event recorded on the legacy default stream (torch's current stream when no side stream is set) that call crashes inside the HIP
    // runtime of ROCm 7.2 (tests/test_gpu_api.py::test_accumulation_on_the_default_stream_then_resolve).
    if (c->accum_pending) { HIP_TRY(hipEventSynchronize(c->ev_accum)); c->accum_pending = false; }
    HIP_TRY(kx::launch_resolve(c->d_accum, c->d_out, c->accum_pixels, c->accum_samples, p->flags, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_out, (size_t)c->accum_pixels * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_ctx_accum_read(MirtContext* c, uint64_t* out_sums, size_t out_len_u64)
{
    if (!c || !out_sums) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    if (!c->d_accum) return fail(MIRT_ERR_NO_SCENE, "nothing accumulated yet");
    if (out_len_u64 < c->accum_pixels * 3) return fail(MIRT_ERR_OUT_BUFFER, "output buffer too small");
    HIP_TRY(hipSetDevice(c->device));
    if (c->accum_pending) HIP_TRY(hipEventSynchronize(c->ev_accum));                 // adds may sit on a caller stream
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_sums, c->d_accum, (size_t)c->accum_pixels * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return MIRT_OK;
}

// ---- adaptive sampling for progressive frames of the resident MIRT_SCENE_HBM scene (include/mirt.h) ----
int mirt_adapt_active(const MirtAdaptPixel* px, const MirtAdaptParams* adapt, uint32_t* out)
{
    if (!px || !adapt || !out) return fail(MIRT_ERR_NULL_POINTER, "pixel/adapt/out is null");
    *out = mirt::adapt_active(px->sum, px->even, px->samples, *adapt) ? 1u : 0u;
    return MIRT_OK;
}

// the blocking calls wait for the last step, on whatever stream it was queued, and fold its time
static int adapt_await(MirtContext* c)
{
    if (c->adapt_pending) {
        HIP_TRY(hipEventSynchronize(c->ev_adapt_end));
        c->adapt_pending = false;
        if (c->adapt_timed) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev_adapt_begin, c->ev_adapt_end));
            c->adapt_ms = ms;
        }
    }
    return MIRT_OK;
}

int mirt_ctx_adapt_reset(MirtContext* c, const MirtParams* p)
{
    int rc = check_params(c, p);
    if (rc != MIRT_OK) return rc;
    if (p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "adaptive sampling exists in path-traced mode only");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t npix = (uint64_t)out_rows(p) * p->width;
    if ((rc = adapt_await(c)) != MIRT_OK) return rc;       // no step may still be running
    c->adapt_pixels = 0;                                   // a failed allocation below leaves no buffer: steps answer MIRT_ERR_OUT_BUFFER
    c->adapt_steps = 0;
    if (!c->ev_adapt_begin) HIP_TRY(hipEventCreate(&c->ev_adapt_begin));
    if (!c->ev_adapt_end) HIP_TRY(hipEventCreate(&c->ev_adapt_end));
    // head 16 bytes | list | block counts | flags
    const uint64_t n_blocks = (npix + 255u) / 256u;
    const size_t off_counts = 16u + (size_t)npix * 4u, off_flags = off_counts + (size_t)n_blocks * 4u;
    const size_t off_log = (off_flags + (size_t)npix + 7u) & ~(size_t)7u, sel_bytes = off_log + MIRT_ADAPT_RUN_MAX_STEPS * sizeof(MirtAdaptRunStep);   // | run log
    c->adapt_run_steps = 0;
    if ((rc = ensure_capacity(&c->d_adapt, &c->cap_adapt, (size_t)npix * sizeof(MirtAdaptPixel))) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_adapt_sel, &c->cap_adapt_sel, sel_bytes)) != MIRT_OK) return rc;
    HIP_TRY(hipMemsetAsync(c->d_adapt, 0, (size_t)npix * sizeof(MirtAdaptPixel), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_adapt_sel, 0, sel_bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->adapt_off_counts = off_counts;
    c->adapt_off_flags = off_flags;
    c->adapt_off_log = off_log;
    c->adapt_pixels = npix;
    c->adapt_width = p->width;
    c->adapt_rows = out_rows(p);
    c->adapt_steps = 0;
    c->adapt_ms = 0.0;
    return MIRT_OK;
}

// What a step (`run`: the steps of a run) is refused for, in the header's order; *q = the params the launch runs with, *pl = its plan, made
// once per call.  Nothing is queued before the last check has passed.
static int check_adapt_step(const MirtContext* c, const MirtParams* p, const MirtAdaptParams* adapt, bool run, MirtParams* q, mirt::QueryPlan* pl)
{
    if (!c || !p || !adapt) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/adapt is null");
    if (!c->have_scene || (!c->hbm && !(adapt->flags & MIRT_ADAPT_LDS)))
        return fail(MIRT_ERR_NO_SCENE, "the context holds no MIRT_SCENE_HBM scene (a scene in LDS takes MIRT_ADAPT_LDS)");
    if (p->mode != MIRT_MODE_PT) return fail(MIRT_ERR_BAD_MODE, "adaptive sampling exists in path-traced mode only");
    if (adapt->flags & ~(uint32_t)(MIRT_ADAPT_POOL | MIRT_ADAPT_LDS)) return fail(MIRT_ERR_BAD_MODE, "unknown MirtAdaptParams.flags bits 0x%x", adapt->flags);
    if (p->flags & (MIRT_FLAG_COUNT_WORK | MIRT_FLAG_COUNT_GRID)) return fail(MIRT_ERR_BAD_MODE, "an adaptive step has no counting build");
    if (p->frame_spp != 0u) return fail(MIRT_ERR_FRAME_SPP, "frame_spp %u: an adaptive step needs independent samples (frame_spp 0)", p->frame_spp);
    *q = *p;
    q->sample_begin = 0;                                    // ignored: every pixel continues its own stream
    const int rc = check_params(c, q);
    if (rc != MIRT_OK) return rc;
    if (p->spp & 1u) return fail(MIRT_ERR_SPP_RANGE, "spp %u is odd: an adaptive step adds to the even and the odd half alike", p->spp);
    if (adapt->max_samples > MIRT_MAX_SPP_PER_CALL)
        return fail(MIRT_ERR_SPP_RANGE, "max_samples %u is out of range: at most %u", adapt->max_samples, (unsigned)MIRT_MAX_SPP_PER_CALL);
    if (!c->d_adapt || c->adapt_pixels == 0 || c->adapt_width != p->width || c->adapt_rows != out_rows(p))
        return fail(MIRT_ERR_OUT_BUFFER, "the adaptive buffer does not match these params: call mirt_ctx_adapt_reset first");
    // the plan: MIRT_ADAPT_POOL where the pool's own limits allow it, otherwise the step without the flag; a scene in LDS needs a layout that fits
    *pl = mirt::plan_adapt(plan_facts(c), c->tuning, *q, adapt->flags, run, c->adapt_pixels);
    if (pl->status != MIRT_OK) return fail(pl->status, "%s", pl->message);
    return MIRT_OK;
}

// A step (run == nullptr) or the run->max_steps steps of a run, queued on one stream between one event pair; `q` and its plan have passed
// check_adapt_step.
static int queue_adapt_steps(MirtContext* c, const MirtParams& q, mirt::QueryPlan pl, const MirtAdaptParams* adapt, const MirtAdaptRun* run, void* hip_stream)
{
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // an MIRT_ADAPT_LDS step runs a persistent grid: its kernel's occupancy bounds the blocks, as a render launch's does (plan_blocks)
    if (pl.family == mirt::kQueryAdaptLds) mirt::query_plan_blocks(pl, kx::blocks_per_cu(kx::query_kernel(pl), pl.threads, pl.lds_bytes));
    mirt::RenderArgs a{};
    fill_common_args(c, &a, q, c->adapt_rows, pinhole_word(c));       // as launch_render
    fill_query_args(c, pl, &a);
    uint32_t* head = reinterpret_cast<uint32_t*>(c->d_adapt_sel);
    uint32_t* list = reinterpret_cast<uint32_t*>(c->d_adapt_sel + 16u);
    const bool timed = c->timing;
    if (timed) HIP_TRY(hipEventRecord(c->ev_adapt_begin, st));
    unsigned char* flags = c->d_adapt_sel + c->adapt_off_flags;
    uint32_t* counts = reinterpret_cast<uint32_t*>(c->d_adapt_sel + c->adapt_off_counts);
    const uint32_t n_steps = run ? run->max_steps : 1u;
    for (uint32_t j = 0; j < n_steps; ++j) {
        // a step of a run: its scan stage chooses the sample count and logs {count, spp}; the render stage reads it from head[1] (10.14).
        // Steps behind an empty one are queued like the others: their select stage finds nothing and their blocks return at once.
        if (run)
            HIP_TRY(kx::launch_adapt_select_run(c->d_adapt, (uint32_t)c->adapt_pixels, *adapt, q.spp, run->min_items, run->max_spp, flags, counts, list, head,
                                                c->d_adapt_sel + c->adapt_off_log + (size_t)j * sizeof(MirtAdaptRunStep), st));
        else
            HIP_TRY(kx::launch_adapt_select(c->d_adapt, (uint32_t)c->adapt_pixels, *adapt, q.spp, flags, counts, list, head, st));
        HIP_TRY(kx::launch_query(pl, a, mirt::QueryBuffers{ nullptr, c->d_adapt, list, head }, st));
    }
    mirt::query_kernel_name(pl, c->last_kernel, sizeof c->last_kernel);
    HIP_TRY(hipEventRecord(c->ev_adapt_end, st));
    c->adapt_pending = true;
    c->adapt_timed = timed;
    c->adapt_ms = 0.0;
    c->adapt_steps += n_steps;
    if (run) c->adapt_run_steps = n_steps;
    return MIRT_OK;
}

int mirt_ctx_adapt_step_device(MirtContext* c, const MirtParams* p, const MirtAdaptParams* adapt, void* hip_stream)
{
    MirtParams q;
    mirt::QueryPlan pl;
    const int rc = check_adapt_step(c, p, adapt, false, &q, &pl);
    if (rc != MIRT_OK) return rc;
    return queue_adapt_steps(c, q, pl, adapt, nullptr, hip_stream);
}

// ---- adaptive runs (include/mirt.h) ----
// what a run's own fields are refused for; spp has passed a step's checks or mirt_adapt_run_spp's
static int check_adapt_run(const MirtAdaptRun* run, uint32_t spp, bool with_steps)
{
    if (run->flags != 0u) return fail(MIRT_ERR_BAD_MODE, "unknown MirtAdaptRun.flags bits 0x%x", run->flags);
    if (with_steps && (run->max_steps == 0u || run->max_steps > MIRT_ADAPT_RUN_MAX_STEPS))
        return fail(MIRT_ERR_BAD_ROWS, "max_steps %u is out of range: 1 .. %u", run->max_steps, (unsigned)MIRT_ADAPT_RUN_MAX_STEPS);
    if (run->max_spp != 0u) {
        uint64_t s = spp;
        while (s < run->max_spp) s <<= 1;
        if (s != run->max_spp || run->max_spp > MIRT_MAX_SPP_PER_CALL)
            return fail(MIRT_ERR_SPP_RANGE, "max_spp %u is neither 0 nor spp %u << m, or above %u", run->max_spp, spp, (unsigned)MIRT_MAX_SPP_PER_CALL);
    }
    return MIRT_OK;
}

int mirt_adapt_run_spp(uint32_t count, uint32_t spp, const MirtAdaptRun* run, uint32_t* out)
{
    if (!run || !out) return fail(MIRT_ERR_NULL_POINTER, "run/out is null");
    if (spp == 0u || (spp & 1u) || spp > MIRT_MAX_SPP_PER_CALL) return fail(MIRT_ERR_SPP_RANGE, "spp %u: a step's size is even, 2 .. %u", spp, (unsigned)MIRT_MAX_SPP_PER_CALL);
    const int rc = check_adapt_run(run, spp, false);
    if (rc != MIRT_OK) return rc;
    *out = mirt::adapt_run_spp(count, spp, run->min_items, run->max_spp);
    return MIRT_OK;
}

int mirt_ctx_adapt_run_device(MirtContext* c, const MirtParams* p, const MirtAdaptParams* adapt, const MirtAdaptRun* run, void* hip_stream)
{
    if (!c || !p || !adapt || !run) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/adapt/run is null");
    MirtParams q;
    mirt::QueryPlan pl;
    int rc = check_adapt_step(c, p, adapt, true, &q, &pl);
    if (rc != MIRT_OK) return rc;
    if ((rc = check_adapt_run(run, q.spp, true)) != MIRT_OK) return rc;
    return queue_adapt_steps(c, q, pl, adapt, run, hip_stream);
}

int mirt_ctx_adapt_run_read(MirtContext* c, MirtAdaptRunStep* out, size_t len, uint32_t* n_steps)
{
    if (!c || !n_steps) return fail(MIRT_ERR_NULL_POINTER, "ctx/n_steps is null");
    if (!c->d_adapt_sel || c->adapt_pixels == 0 || c->adapt_run_steps == 0) return fail(MIRT_ERR_NO_SCENE, "no adaptive run has been queued since the reset");
    *n_steps = c->adapt_run_steps;
    if (len < c->adapt_run_steps) return fail(MIRT_ERR_OUT_BUFFER, "the log holds %u steps, room for %zu", c->adapt_run_steps, len);
    if (!out) return fail(MIRT_ERR_NULL_POINTER, "out is null");
    HIP_TRY(hipSetDevice(c->device));
    const int rc = adapt_await(c);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipMemcpy(out, c->d_adapt_sel + c->adapt_off_log, sizeof(MirtAdaptRunStep) * (size_t)c->adapt_run_steps, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

static int check_adapt_resolve(const MirtContext* c, const MirtParams* p, const void* out, size_t out_len)
{
    if (!c || !p || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/out is null");
    if (!c->d_adapt || c->adapt_pixels == 0 || c->adapt_steps == 0) return fail(MIRT_ERR_NO_SCENE, "no adaptive step has run since the reset");
    if (out_len < c->adapt_pixels * 4) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %llu needed", out_len, (unsigned long long)c->adapt_pixels * 4);
    return MIRT_OK;
}

int mirt_ctx_adapt_resolve_device(MirtContext* c, const MirtParams* p, void* d_out, size_t out_len, void* hip_stream)
{
    const int rc = check_adapt_resolve(c, p, d_out, out_len);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(kx::launch_adapt_resolve(c->d_adapt, (uint32_t*)d_out, c->adapt_pixels, p->flags, hip_stream ? (hipStream_t)hip_stream : c->stream));
    return MIRT_OK;
}

int mirt_ctx_adapt_resolve(MirtContext* c, const MirtParams* p, uint8_t* out, size_t out_len)
{
    int rc = check_adapt_resolve(c, p, out, out_len);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_capacity(&c->d_out, &c->cap_out, (size_t)c->adapt_pixels)) != MIRT_OK) return rc;
    if ((rc = adapt_await(c)) != MIRT_OK) return rc;       // the HOST waits for a step on a caller stream (see mirt_ctx_accum_resolve)
    HIP_TRY(kx::launch_adapt_resolve(c->d_adapt, c->d_out, c->adapt_pixels, p->flags, c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_out, (size_t)c->adapt_pixels * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_ctx_adapt_read(MirtContext* c, MirtAdaptPixel* out, size_t len)
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    if (!c->d_adapt || c->adapt_pixels == 0) return fail(MIRT_ERR_NO_SCENE, "no adaptive buffer: call mirt_ctx_adapt_reset first");
    if (len < c->adapt_pixels) return fail(MIRT_ERR_OUT_BUFFER, "the buffer holds %llu records, room for %zu", (unsigned long long)c->adapt_pixels, len);
    HIP_TRY(hipSetDevice(c->device));
    const int rc = adapt_await(c);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_adapt, (size_t)c->adapt_pixels * sizeof(MirtAdaptPixel), hipMemcpyDeviceToHost));
    return MIRT_OK;
}

int mirt_ctx_adapt_write(MirtContext* c, const MirtAdaptPixel* in, size_t len)
{
    if (!c || !in) return fail(MIRT_ERR_NULL_POINTER, "ctx/in is null");
    if (!c->d_adapt || c->adapt_pixels == 0) return fail(MIRT_ERR_NO_SCENE, "no adaptive buffer: call mirt_ctx_adapt_reset first");
    if (len != c->adapt_pixels) return fail(MIRT_ERR_OUT_BUFFER, "the buffer holds %llu records, %zu given", (unsigned long long)c->adapt_pixels, len);
    HIP_TRY(hipSetDevice(c->device));
    const int rc = adapt_await(c);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->d_adapt, in, (size_t)c->adapt_pixels * sizeof(MirtAdaptPixel), hipMemcpyHostToDevice));
    return MIRT_OK;
}

int mirt_ctx_adapt_list_read(MirtContext* c, uint32_t* list, size_t len, uint32_t* count)
{
    if (!c || !count) return fail(MIRT_ERR_NULL_POINTER, "ctx/count is null");
    if (!c->d_adapt_sel || c->adapt_steps == 0) return fail(MIRT_ERR_NO_SCENE, "no adaptive step has run since the reset");
    HIP_TRY(hipSetDevice(c->device));
    const int rc = adapt_await(c);
    if (rc != MIRT_OK) return rc;
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, c->d_adapt_sel, sizeof n, hipMemcpyDeviceToHost));
    *count = n;
    if (len < n) return fail(MIRT_ERR_OUT_BUFFER, "the list holds %u indices, room for %zu", n, len);
    if (n && !list) return fail(MIRT_ERR_NULL_POINTER, "list is null");
    if (n) HIP_TRY(hipMemcpy(list, c->d_adapt_sel + 16u, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

int mirt_ctx_adapt_stats(MirtContext* c, MirtAdaptStats* out)
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    *out = MirtAdaptStats{};
    if (!c->d_adapt_sel || c->adapt_pixels == 0) return MIRT_OK;       // all 0 before the first reset
    HIP_TRY(hipSetDevice(c->device));
    const int rc = adapt_await(c);
    if (rc != MIRT_OK) return rc;
    unsigned long long head[2] = { 0, 0 };
    HIP_TRY(hipMemcpy(head, c->d_adapt_sel, sizeof head, hipMemcpyDeviceToHost));
    out->pixels = c->adapt_pixels;
    out->total_samples = head[1];
    out->active = (uint32_t)head[0];
    out->steps = c->adapt_steps;
    out->kernel_ms = c->adapt_ms;
    return MIRT_OK;
}

// ---- the a-trous filter over the accumulation or the adaptive records (include/mirt.h) ----
// What both entry points check, in the header's order; inv[i] = level i's 1 / sg^2 (all 1 for sigma_colour == 0, where nothing reads them).
// Nothing is queued, and no scratch grown, before the last check has passed.
static int check_denoise(const MirtContext* c, const MirtParams* p, const MirtDenoiseParams* d, const void* guides, size_t guides_len, const void* out,
                         size_t out_len, float inv[8])
{
    if (!c || !p || !d || !guides || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/denoise/guides/out is null");
    if (d->source > MIRT_DENOISE_SRC_ADAPT) return fail(MIRT_ERR_BAD_MODE, "unknown MirtDenoiseParams.source %u", d->source);
    if (d->flags & ~(uint32_t)MIRT_DENOISE_OUT_F32) return fail(MIRT_ERR_BAD_MODE, "unknown MirtDenoiseParams.flags bits 0x%x", d->flags);
    if (d->levels < 1u || d->levels > 8u) return fail(MIRT_ERR_BAD_MODE, "levels %u is outside 1..8", d->levels);
    if (d->normal_log2 > 8u) return fail(MIRT_ERR_BAD_MODE, "normal_log2 %u is above 8", d->normal_log2);
    if (!(d->sigma_colour >= 0.0f)) return fail(MIRT_ERR_BAD_MODE, "sigma_colour %g is negative or NaN", (double)d->sigma_colour);
    for (uint32_t i = 0; i < 8u; ++i) inv[i] = 1.0f;
    if (d->sigma_colour > 0.0f)
        for (uint32_t i = 0; i < d->levels; ++i) {
            const float sg = d->sigma_colour * std::ldexp(1.0f, -(int)i);      // float32, one operation each
            inv[i] = 1.0f / (sg * sg);
            if (!(inv[i] > 0.0f) || !std::isfinite(inv[i]))
                return fail(MIRT_ERR_BAD_MODE, "sigma_colour %g: level %u's 1 / sg^2 is not finite and positive", (double)d->sigma_colour, i);
        }
    if (p->n_parts > 1u && p->tile_rows != 0u)
        return fail(MIRT_ERR_BAD_ROWS, "a tile partition (part %u/%u, %u rows per tile): its compact rows are not neighbours in the image", p->part, p->n_parts, p->tile_rows);
    const bool adapt = d->source == MIRT_DENOISE_SRC_ADAPT;
    const uint64_t npix = adapt ? c->adapt_pixels : c->accum_pixels;
    const uint32_t width = adapt ? c->adapt_width : c->accum_width, rows = adapt ? c->adapt_rows : c->accum_rows;
    if (!(adapt ? (const void*)c->d_adapt : (const void*)c->d_accum) || npix == 0u)
        return fail(MIRT_ERR_OUT_BUFFER, "no %s buffer: call %s first", adapt ? "adaptive" : "accumulation", adapt ? "mirt_ctx_adapt_reset" : "mirt_ctx_accum_reset");
    if (p->width != width || out_rows(p) != rows) return fail(MIRT_ERR_OUT_BUFFER, "the %s buffer does not match these params: %u x %u at its reset",
                                                              adapt ? "adaptive" : "accumulation", width, rows);
    if (guides_len / sizeof(MirtFeaturePixel) < npix) return fail(MIRT_ERR_OUT_BUFFER, "the guides hold %zu bytes, %llu needed", guides_len,
                                                                  (unsigned long long)npix * sizeof(MirtFeaturePixel));
    const size_t px_bytes = (d->flags & MIRT_DENOISE_OUT_F32) ? 16u : 4u;
    if (out_len / px_bytes < npix) return fail(MIRT_ERR_OUT_BUFFER, "output buffer holds %zu bytes, %llu needed", out_len, (unsigned long long)npix * px_bytes);
    if (adapt ? c->adapt_steps == 0u : c->accum_samples == 0u)
        return fail(MIRT_ERR_NO_SCENE, adapt ? "no adaptive step has run since the reset" : "nothing accumulated yet");
    return MIRT_OK;
}

// The levels that run the staged shape, bit i = level i: by measurement at 1920 x 1080 staging wins up to step 8 (by 32,
// 30, 21 and 8 us per level) and loses from step 16 on (by 12 and 35 us), where a class's staging loads are 256 bytes and more apart.
constexpr uint32_t kDenoiseStagedLevels = 0x0fu;

// Queue the prepare kernel and the levels on `st`.  No host synchronisation unless the scratch must grow.  An ACCUM denoise is a reading link
// of the frame chain (launch_frame with spp == 0); the event pair and the pending flag are the ray queries' (mirt_ctx_trace_stats folds the time).
static int launch_denoise(MirtContext* c, const MirtParams* p, const MirtDenoiseParams* d, const float inv[8], const void* d_guides, void* d_out, hipStream_t st)
{
    const bool adapt = d->source == MIRT_DENOISE_SRC_ADAPT;
    const uint64_t npix = adapt ? c->adapt_pixels : c->accum_pixels;
    const size_t need = (size_t)npix * 48u;                     // two colour planes and the guide plane
    if (need > c->cap_denoise || !c->d_denoise) {
        HIP_TRY(hipDeviceSynchronize());                        // an earlier denoise, on whatever stream, may still use the planes freed here
        const int rc = ensure_capacity(&c->d_denoise, &c->cap_denoise, need);
        if (rc != MIRT_OK) return rc;
    }
    if (!adapt) { const int rc = order_frame(c, st); if (rc != MIRT_OK) return rc; }
    const bool timed = c->timing;
    if (timed) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
    const bool f32_out = (d->flags & MIRT_DENOISE_OUT_F32) != 0u;
    const uint32_t staged = c->tuning.denoise_staged >= 0 ? (uint32_t)c->tuning.denoise_staged : kDenoiseStagedLevels;
    HIP_TRY(kx::launch_denoise(d->source, adapt ? (const void*)c->d_adapt : (const void*)c->d_accum, c->accum_samples, d_guides,
                               adapt ? c->adapt_width : c->accum_width, adapt ? c->adapt_rows : c->accum_rows, d->levels, d->normal_log2,
                               d->sigma_colour != 0.0f, inv, f32_out, p->flags & (MIRT_FLAG_NO_TONEMAP | MIRT_FLAG_NO_SRGB), staged, c->d_denoise, d_out, st));
    snprintf(c->last_kernel, sizeof c->last_kernel, "denoise_atrous_%skernel<%s>", ((staged >> (d->levels - 1u)) & 1u) ? "staged_" : "", f32_out ? "f32" : "rgba8");
    HIP_TRY(hipEventRecord(c->ev_trace_end, st));
    c->trace_pending = true;
    c->trace_timed = timed;
    c->trace_counted = false;
    c->trace_stats = MirtRayStats{};
    if (!adapt) {
        c->accum_stream = st;                               // the next frame, on whatever stream, is ordered after this read (order_frame)
        if (st != c->stream) {                              // mirt_ctx_accum_reset / _resolve / _read must not overtake it (launch_frame)
            HIP_TRY(hipEventRecord(c->ev_accum, st));
            c->accum_pending = true;
            if (std::find(c->untimed_streams.begin(), c->untimed_streams.end(), st) == c->untimed_streams.end()) c->untimed_streams.push_back(st);
        }
    }
    return MIRT_OK;
}

int mirt_ctx_denoise_device(MirtContext* c, const MirtParams* p, const MirtDenoiseParams* d, const void* d_guides, size_t guides_len, void* d_out, size_t out_len,
                            void* hip_stream)
{
    float inv[8];
    const int rc = check_denoise(c, p, d, d_guides, guides_len, d_out, out_len, inv);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_denoise(c, p, d, inv, d_guides, d_out, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_denoise(MirtContext* c, const MirtParams* p, const MirtDenoiseParams* d, const MirtFeaturePixel* guides, size_t guides_len, void* out, size_t out_len)
{
    float inv[8];
    int rc = check_denoise(c, p, d, guides, guides_len, out, out_len, inv);
    if (rc != MIRT_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool adapt = d->source == MIRT_DENOISE_SRC_ADAPT;
    const size_t npix = (size_t)(adapt ? c->adapt_pixels : c->accum_pixels);
    const size_t g_bytes = npix * sizeof(MirtFeaturePixel), o_bytes = npix * ((d->flags & MIRT_DENOISE_OUT_F32) ? 16u : 4u);
    // the guides are staged where a host trace stages its hits, the result where it stages its rays
    if ((rc = ensure_capacity(&c->d_trace_hits, &c->cap_trace_hits, g_bytes)) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_trace_rays, &c->cap_trace_rays, o_bytes)) != MIRT_OK) return rc;
    if (adapt && (rc = adapt_await(c)) != MIRT_OK) return rc;      // the HOST waits for a step on a caller stream (see mirt_ctx_adapt_resolve)
    if (!adapt && c->accum_pending) { HIP_TRY(hipEventSynchronize(c->ev_accum)); c->accum_pending = false; }      // ... and for an add (see mirt_ctx_accum_resolve)
    HIP_TRY(hipMemcpyAsync(c->d_trace_hits, guides, g_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_denoise(c, p, d, inv, c->d_trace_hits, c->d_trace_rays, c->stream)) != MIRT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->d_trace_rays, o_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

// ---- temporal reprojection of a denoised frame by first-hit depth and id (include/mirt.h) ----
static bool ranges_overlap(const void* a, uint64_t a_len, const void* b, uint64_t b_len)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a_len != 0u && b_len != 0u && x < y + b_len && y < x + a_len;
}

// What both entry points check, in the header's order; *rb: the band's first image row, *rows: its rows (0: nothing to do).
static int check_reproject(const MirtContext* c, const MirtParams* p, const MirtReprojectParams* r, const MirtReprojectFrames* f, uint32_t* rb, uint32_t* rows)
{
    if (!c || !p || !r || !f) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/reproject/frames is null");
    if (!f->colour || !f->guides || !f->prev_colour || !f->prev_guides || !f->out)
        return fail(MIRT_ERR_NULL_POINTER, "colour/guides/prev_colour/prev_guides/out is null");
    if (r->flags & ~(uint32_t)MIRT_REPROJECT_CLAMP) return fail(MIRT_ERR_BAD_MODE, "unknown MirtReprojectParams.flags bits 0x%x", r->flags);
    if (!(r->max_history >= 1.0f) || !std::isfinite(r->max_history)) return fail(MIRT_ERR_BAD_MODE, "max_history %g is not finite and >= 1", (double)r->max_history);
    if (!(r->depth_tolerance >= 0.0f) || !std::isfinite(r->depth_tolerance))
        return fail(MIRT_ERR_BAD_MODE, "depth_tolerance %g is not finite and >= 0", (double)r->depth_tolerance);
    if (p->width == 0 || p->height == 0)
        return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", p->width, p->height);
    uint32_t re;
    if (!rows_valid(p, rb, &re)) return fail(MIRT_ERR_BAD_ROWS, "invalid row selection [%u,%u) of %u, part %u/%u", p->row_begin, p->row_end, p->height, p->part, p->n_parts);
    if (p->n_parts > 1u && p->tile_rows != 0u)
        return fail(MIRT_ERR_BAD_ROWS, "a tile partition (part %u/%u, %u rows per tile): its compact rows are not neighbours in the image", p->part, p->n_parts, p->tile_rows);
    *rows = out_rows(p);
    const uint64_t n = f->pixels;
    if (n < (uint64_t)*rows * p->width) return fail(MIRT_ERR_OUT_BUFFER, "the frames hold %llu records, %llu needed", (unsigned long long)n, (unsigned long long)*rows * p->width);
    const void* in[4] = { f->colour, f->guides, f->prev_colour, f->prev_guides };
    const uint64_t in_len[4] = { n * 16u, n * sizeof(MirtFeaturePixel), n * 16u, n * sizeof(MirtFeaturePixel) };
    for (int i = 0; i < 4; ++i)
        if (ranges_overlap(f->out, n * 16u, in[i], in_len[i]) || (f->out_rgba8 && ranges_overlap(f->out_rgba8, n * 4u, in[i], in_len[i])))
            return fail(MIRT_ERR_OUT_BUFFER, "out or out_rgba8 overlaps an input plane");
    if (f->out_rgba8 && ranges_overlap(f->out, n * 16u, f->out_rgba8, n * 4u)) return fail(MIRT_ERR_OUT_BUFFER, "out and out_rgba8 overlap");
    return MIRT_OK;
}

// Queue reproject_kernel on `st`: no scratch, no host synchronisation.  The event pair and the pending flag are the ray queries'
// (mirt_ctx_trace_stats folds the time); the launch ring, MirtStats and the accumulation stay as they are.
static int launch_reproject(MirtContext* c, const MirtParams* p, const MirtReprojectParams* r, uint32_t rb, uint32_t rows, const void* d_colour, const void* d_guides,
                            const void* d_prev_colour, const void* d_prev_guides, void* d_out, void* d_rgba8, hipStream_t st)
{
    kx::ReprojectArgs a{};
    a.previous = r->previous; a.current = r->current;
    a.width = p->width; a.height = p->height; a.row_begin = rb; a.rows = rows;
    a.flags = p->flags & (MIRT_FLAG_NO_TONEMAP | MIRT_FLAG_NO_SRGB);
    a.max_history = r->max_history; a.depth_tolerance = r->depth_tolerance;
    const bool clamp = (r->flags & MIRT_REPROJECT_CLAMP) != 0u;
    const bool timed = c->timing;
    if (timed) HIP_TRY(hipEventRecord(c->ev_trace_begin, st));
    HIP_TRY(kx::launch_reproject(a, clamp, d_colour, d_guides, d_prev_colour, d_prev_guides, d_out, d_rgba8, st));
    snprintf(c->last_kernel, sizeof c->last_kernel, "reproject_kernel<%s,%s>", clamp ? "true" : "false", d_rgba8 ? "true" : "false");
    HIP_TRY(hipEventRecord(c->ev_trace_end, st));
    c->trace_pending = true;
    c->trace_timed = timed;
    c->trace_counted = false;
    c->trace_stats = MirtRayStats{};
    return MIRT_OK;
}

int mirt_ctx_reproject_device(MirtContext* c, const MirtParams* p, const MirtReprojectParams* r, const MirtReprojectFrames* f, void* hip_stream)
{
    uint32_t rb = 0, rows = 0;
    const int rc = check_reproject(c, p, r, f, &rb, &rows);
    if (rc != MIRT_OK || rows == 0u) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_reproject(c, p, r, rb, rows, f->colour, f->guides, f->prev_colour, f->prev_guides, f->out, f->out_rgba8, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int mirt_ctx_reproject(MirtContext* c, const MirtParams* p, const MirtReprojectParams* r, const MirtReprojectFrames* f)
{
    uint32_t rb = 0, rows = 0;
    int rc = check_reproject(c, p, r, f, &rb, &rows);
    if (rc != MIRT_OK || rows == 0u) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the four input planes are staged where a host trace stages its hits, the two results where it stages its rays
    const size_t n = (size_t)rows * p->width, c_bytes = n * 16u, g_bytes = n * sizeof(MirtFeaturePixel);
    if ((rc = ensure_capacity(&c->d_trace_hits, &c->cap_trace_hits, 2u * (c_bytes + g_bytes))) != MIRT_OK) return rc;
    if ((rc = ensure_capacity(&c->d_trace_rays, &c->cap_trace_rays, c_bytes + n * 4u)) != MIRT_OK) return rc;
    unsigned char* in = reinterpret_cast<unsigned char*>(c->d_trace_hits);
    unsigned char* out = reinterpret_cast<unsigned char*>(c->d_trace_rays);
    unsigned char *d_colour = in, *d_guides = in + c_bytes, *d_prev_colour = d_guides + g_bytes, *d_prev_guides = d_prev_colour + c_bytes;
    HIP_TRY(hipMemcpyAsync(d_colour, f->colour, c_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_guides, f->guides, g_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_prev_colour, f->prev_colour, c_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_prev_guides, f->prev_guides, g_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_reproject(c, p, r, rb, rows, d_colour, d_guides, d_prev_colour, d_prev_guides, out, f->out_rgba8 ? out + c_bytes : nullptr, c->stream)) != MIRT_OK)
        return rc;
    HIP_TRY(hipMemcpyAsync(f->out, out, c_bytes, hipMemcpyDeviceToHost, c->stream));
    if (f->out_rgba8) HIP_TRY(hipMemcpyAsync(f->out_rgba8, out + c_bytes, n * 4u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MIRT_OK;
}

int mirt_camera_project(const MirtGpuCamera* cam, uint32_t width, uint32_t height, const float point[3], float out[3])
{
    if (!cam || !point || !out) return fail(MIRT_ERR_NULL_POINTER, "camera/point/out is null");
    if (width == 0 || height == 0) return fail(MIRT_ERR_VIEWPORT_SIZE, "viewport_size elements cannot be zero: (%u, %u)", width, height);
    // reproject_pixel's lines rel .. fy with `cam` as the previous camera, operation for operation (this file is compiled with
    // -ffp-contract=off)
    const float* H = cam->horizontal;
    const float* V = cam->vertical;
    float rel[3], a[3], q[3];
    for (int k = 0; k < 3; ++k) {
        rel[k] = point[k] - cam->eye[k];
        a[k] = cam->lower_left_corner[k] - cam->eye[k];
    }
    const float n[3] = { H[1] * V[2] - H[2] * V[1], H[2] * V[0] - H[0] * V[2], H[0] * V[1] - H[1] * V[0] };
    auto dot = [](const float* x, const float* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; };
    const float s = dot(rel, n) / dot(a, n);
    for (int k = 0; k < 3; ++k) q[k] = rel[k] / s - a[k];
    const float pu = dot(q, H) / dot(H, H), pv = dot(q, V) / dot(V, V);
    out[0] = pu * (float)width - 0.5f;
    out[1] = (1.0f - pv) * (float)height - 0.5f;
    out[2] = s;
    return MIRT_OK;
}

int mirt_ctx_selftest_math(MirtContext* c, uint64_t out[2])
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = mirt_ctx_synchronize(c); if (rc != MIRT_OK) return rc; }    // borrows counter block 0
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_TRY(kx::launch_selftest_math(c->d_counters, c->stream));
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out[0] = h[0];
    out[1] = h[1];
    return MIRT_OK;
}

int mirt_ctx_selftest_checker_sign(MirtContext* c, uint64_t out[3])
{
    if (!c || !out) return fail(MIRT_ERR_NULL_POINTER, "ctx/out is null");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = mirt_ctx_synchronize(c); if (rc != MIRT_OK) return rc; }    // borrows counter block 0
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, 3 * sizeof(unsigned long long), c->stream));
    HIP_TRY(kx::launch_selftest_checker_sign(c->d_counters, c->stream));
    unsigned long long h[3] = { 0, 0, 0 };
    HIP_TRY(hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, 3 * sizeof(unsigned long long), c->stream));      // the block goes back as it came
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return MIRT_OK;
}

int mirt_render(const MirtScene* scene, const MirtParams* params, int device, uint8_t* out, size_t out_len)
{
    MirtContext* c = nullptr;
    int rc = mirt_ctx_create(device, &c);
    if (rc != MIRT_OK) return rc;
    rc = mirt_ctx_set_scene(c, scene);
    if (rc == MIRT_OK) rc = mirt_ctx_render(c, params, out, out_len);
    mirt_ctx_destroy(c);
    return rc;
}

int mirt_rgba8_to_rgb8(const uint8_t* rgba, size_t n_pixels, uint8_t* rgb)
{
    if (!rgba || !rgb) return fail(MIRT_ERR_NULL_POINTER, "rgba/rgb is null");
    for (size_t i = 0; i < n_pixels; ++i) {
        rgb[3 * i + 0] = rgba[4 * i + 0];
        rgb[3 * i + 1] = rgba[4 * i + 1];
        rgb[3 * i + 2] = rgba[4 * i + 2];
    }
    return MIRT_OK;
}

int mirt_ctx_deinterleave_device(MirtContext* c, const MirtParams* p, const void* d_parts, size_t part_stride,
                                 void* d_out, size_t out_len, void* hip_stream)
{
    if (!c || !p || !d_parts || !d_out) return fail(MIRT_ERR_NULL_POINTER, "ctx/params/buffers is null");
    uint32_t rb, re;
    if (p->width == 0 || p->height == 0 || !rows_valid(p, &rb, &re)) return fail(MIRT_ERR_BAD_ROWS, "invalid row selection");
    if (p->tile_rows == 0 || p->n_parts <= 1) return fail(MIRT_ERR_BAD_ROWS, "params describe no tile interleave");
    const uint32_t band = re - rb;
    if (out_len < (size_t)band * p->width * 4) return fail(MIRT_ERR_OUT_BUFFER, "output buffer too small");
    if (part_stride % 4 != 0) return fail(MIRT_ERR_OUT_BUFFER, "part_stride must be a multiple of 4 bytes");
    MirtParams q = *p;
    uint32_t max_rows = 0;
    for (uint32_t i = 0; i < p->n_parts; ++i) { q.part = i; const uint32_t r = out_rows(&q); if (r > max_rows) max_rows = r; }
    if (part_stride < (size_t)max_rows * p->width * 4) return fail(MIRT_ERR_OUT_BUFFER, "part_stride smaller than the largest part");
    HIP_TRY(hipSetDevice(c->device));
    mirt::AssembleArgs d{};
    d.parts[0] = (const uint32_t*)d_parts; d.out = (uint32_t*)d_out; d.part_stride_px = part_stride / 4;
    d.width = p->width; d.band_rows = band; d.tile_rows = p->tile_rows; d.n_parts = p->n_parts;
    d.vec4 = (p->width % 4 == 0 && part_stride % 16 == 0 && (uintptr_t)d_parts % 16 == 0 && (uintptr_t)d_out % 16 == 0) ? 1u : 0u;
    HIP_TRY(kx::launch_assemble(d, mirt::LaunchOn(hip_stream ? (hipStream_t)hip_stream : c->stream)));
    return MIRT_OK;
}

}  // extern "C"

int mirt::check_accum_frame(const MirtContext* ctx, const MirtParams* params)
{
    MirtParams q;
    return check_frame_params(ctx, params, &q);
}
