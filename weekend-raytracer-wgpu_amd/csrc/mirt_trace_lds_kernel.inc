// mirt_trace_lds_kernel.inc -- ray queries against a scene that lives in LDS (MIRT_QUERY_LDS in the flags of mirt_ctx_trace_rays*;
// include/mirt.h, DESIGN.md 10.16).  Included once by mirt_kernels.hip behind the MIRT_SCENE_HBM query kernels, whose vector types it
// shares; exact build only.
//
// trace_rays_lds_kernel<GRID, ANY, COUNT>: the shape of adapt_pixels_lds_kernel (mirt_adapt_lds_kernel.inc) -- 256-thread blocks whose
// four waves share ONE staged scene, a persistent grid of min(ceil(rays / 256), CUs x resident blocks) blocks whose waves stride over
// units of 64 consecutive rays, unit = blockIdx.x * 4 + wave, + gridDim.x * 4: lane = ray, the wave composition of trace_rays_kernel.
// A block whose first unit does not exist returns before anything is staged; in a live block every wave passes the staging barriers and
// there is no block barrier behind them (mirt_lds_block_text.inc).  The ray load, the flat scan and the hit record are the parts of
// mirt_trace_ray_text.inc that trace_rays_kernel includes; `closest` starts at the ray's t_max.
//   GRID = false: that flat scan over the STAGED sphere table: test_sphere in original index order, ANY with the same early exit, so
//                 the per-lane counters are the twin's.
//   GRID = true : nearest_hit_grid_query below.
//   COUNT       : Work<true>, flushed once per wave at its end: rays, the sphere tests a lane really performs, roots, rays with a hit;
//                 on the grid also cells visited per lane / cell-loop iterations per wave (MirtRayStats.nodes / wave_nodes).

constexpr uint32_t kQueryLdsMinWaves = 4;      // waves per SIMD the LDS query builds are held to (launch bounds), as kAdaptLdsMinWaves

// Which rays the grid walk is trusted with, as a pure function of the ray's direction.  The walk's proof (the comment above GridLds) is
// about rounding: every step of the clip and of the DDA is a product or quotient with a relative error of a few u, which holds while
// nothing overflows, underflows or is NaN.  A component is therefore either exactly zero (its axis takes no part) or finite with
// 2^-40 <= |d| <= 2^40: then a = |d|^2 lies in [2^-80, 2^82], 1 / d_k and 1 / a are normal numbers, and crossing parameters
// (a coordinate difference over d_k) stay far from the format's ends for every scene mirt_ctx_set_scene accepts.  The length of the
// direction does not matter inside that range -- t scales with 1 / |d| and t x d does not change --, so a ray 1e-3 long whose hits lie
// at t > 1000 walks.  Every other direction (NaN, infinite, denormal, absurdly long or short components) scans every record in id
// order, as far-origin rays do: that IS the flat scan, by test_sphere's (f, id) tie-break.
MIRT_DEV bool query_walk_trusts(f3 rd)
{
    const float lo = 0x1p-40f, hi = 0x1p40f;
    const float ax = abs_(rd.x), ay = abs_(rd.y), az = abs_(rd.z);
    const bool okx = (rd.x == 0.0f) | ((ax >= lo) & (ax <= hi));          // a NaN fails both comparisons
    const bool oky = (rd.y == 0.0f) | ((ay >= lo) & (ay <= hi));
    const bool okz = (rd.z == 0.0f) | ((az >= lo) & (az <= hi));
    return okx & oky & okz;
}

// nearest_hit_grid for a caller's ray: `closest` starts at t_max -- which may be larger than kMaxT, infinite, negative or NaN -- and the
// walk is bounded by the grid's box (tmax starts at the largest finite float, not at kMaxT) and by the running `closest`.  A variant of
// its own, so that the render kernels keep their code objects.
// Equivalence: the argument above GridLds, with t_max in kMaxT's place -- the scan replaces `closest` exactly when f < closest, the
// walk may stop once closest <= the parameter at which the ray leaves the current cell, and a sphere with a smaller f is listed in a
// cell already visited.  A NaN t_max takes no hit in either scan (every comparison with it is false); a t_max <= MIN_T neither.
// Rays the proof does not cover do not walk: query_walk_trusts (direction) and the far-origin guard (origin; NaN and infinite origins
// fail `dist2 <= guard` and so count as far).  Untrusted directions scan EVERY record; far origins as in nearest_hit_grid.
// Termination, for every bit pattern: the walk's loop moves each walking lane's cell index by exactly one, along one axis, in a
// direction (sx, sy, sz) fixed before the loop -- whatever tx, ty, tz hold, NaN included, one of the three selects is taken -- and the
// lane leaves the loop when an index leaves [0, dim): at most dims[0] + dims[1] + dims[2] iterations.  The first cell is clamped into
// the grid after the float -> int conversion (which saturates, NaN -> 0).  The scans run n_spheres and n_big iterations, a cell's item
// loop at most its 16-bit count.
// ANY: a lane stops at its first hit, wherever it finds it; whether one exists does not depend on the order.
template <bool COUNT, bool ANY, bool FLATY>
MIRT_DEV int nearest_hit_grid_query(const GridLds& G, f3 ro, f3 rd, float t_max, bool alive, float& closest_out, Work<COUNT>& work, uint32_t lane)
{
    const float a = dot(rd, rd);
    const float inv_a = rcp_(a);
    float closest = t_max;
    int best = -1;
    const GridHeader& H = *G.h;
    if (alive) work.add(kCntRays);
    bool go = alive;
    if constexpr (ANY) {
        const uint32_t n_big = H.n_big;
        for (uint32_t j = 0; j < n_big; ++j) {
            test_sphere<COUNT>(G.big_recs[j], G.big[j], ro, rd, a, inv_a, go, closest, best, work);
            go = go && best < 0;
            if (!ballot_(go)) break;
        }
    } else {
        test_big_spheres<COUNT>(G, ro, rd, a, inv_a, go, closest, best, work);
    }

    // clip the ray against the grid's box
    const f3 org = mk(H.org[0], H.org[1], H.org[2]);
    const f3 cell = mk(H.cell[0], H.cell[1], H.cell[2]);
    const f3 inv_cell = mk(H.inv_cell[0], H.inv_cell[1], H.inv_cell[2]);
    const int dx = (int)H.dims[0], dy = (int)H.dims[1], dz = (int)H.dims[2];
    const f3 hi = mk(fma_((float)dx, cell.x, org.x), fma_((float)dy, cell.y, org.y), fma_((float)dz, cell.z, org.z));
    const float kHuge = 3.0e38f;
    const f3 inv_d = mk(rd.x != 0.0f ? rcp_(rd.x) : kHuge, rd.y != 0.0f ? rcp_(rd.y) : kHuge, rd.z != 0.0f ? rcp_(rd.z) : kHuge);
    float tmin = 0.0f, tmax = kHuge;
    bool inside = go;
    {
        const float o[3] = { ro.x, ro.y, ro.z }, d[3] = { rd.x, rd.y, rd.z }, id[3] = { inv_d.x, inv_d.y, inv_d.z };
        const float lo3[3] = { org.x, org.y, org.z }, hi3[3] = { hi.x, hi.y, hi.z };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool nz = d[k] != 0.0f;
            const float ta = (lo3[k] - o[k]) * id[k], tb = (hi3[k] - o[k]) * id[k];
            const float t_lo = (ta < tb) ? ta : tb, t_hi = (ta < tb) ? tb : ta;
            tmin = nz ? max_(tmin, t_lo) : tmin;
            tmax = (nz & (t_hi < tmax)) ? t_hi : tmax;
            inside = inside & (nz | ((o[k] >= lo3[k]) & (o[k] <= hi3[k])));
        }
    }
    bool walking = inside && (tmin <= tmax) && (tmin < closest);
    // rays that do not trust the walk: an untrusted direction scans every record; a far origin does if it can reach the grid at all
    const float4 gd = *reinterpret_cast<const float4*>(H.guard);
    const f3 qc = ro - mk(gd.x, gd.y, gd.z);
    const float dist2 = dot(qc, qc);
    const bool odd = go & !query_walk_trusts(rd);
    const bool far = go & !(dist2 <= gd.w);
    if (ballot_(odd | far)) {
        bool scan = odd || (far && far_ray_reaches(ro, rd, org, hi, dist2, H.bound_r));
        walking = walking & !(odd | far);
        const uint32_t n_rec = __builtin_amdgcn_readfirstlane(H.n_spheres);
        for (uint32_t i = 0; i < n_rec; ++i) {
            if (!ballot_(scan)) break;
            test_sphere<COUNT>(G.recs[i], i, ro, rd, a, inv_a, scan, closest, best, work);
            if constexpr (ANY) scan = scan && best < 0;
        }
    }
    if constexpr (ANY) walking = walking && best < 0;
    const f3 p0 = fma3(tmin, rd, ro);
    int cx = (int)((p0.x - org.x) * inv_cell.x), cy = 0, cz = (int)((p0.z - org.z) * inv_cell.z);
    cx = cx < 0 ? 0 : (cx >= dx ? dx - 1 : cx);
    cz = cz < 0 ? 0 : (cz >= dz ? dz - 1 : cz);
    if constexpr (!FLATY) { cy = (int)((p0.y - org.y) * inv_cell.y); cy = cy < 0 ? 0 : (cy >= dy ? dy - 1 : cy); }
    const int sx = rd.x > 0.0f ? 1 : -1, sy = rd.y > 0.0f ? 1 : -1, sz = rd.z > 0.0f ? 1 : -1;
    float tx = rd.x != 0.0f ? (fma_((float)(cx + (sx > 0 ? 1 : 0)), cell.x, org.x) - ro.x) * inv_d.x : kHuge;
    float tz = rd.z != 0.0f ? (fma_((float)(cz + (sz > 0 ? 1 : 0)), cell.z, org.z) - ro.z) * inv_d.z : kHuge;
    const float ddx = rd.x != 0.0f ? abs_(cell.x * inv_d.x) : kHuge;
    const float ddz = rd.z != 0.0f ? abs_(cell.z * inv_d.z) : kHuge;
    float ty = kHuge, ddy = kHuge;
    if constexpr (!FLATY) {
        ty = rd.y != 0.0f ? (fma_((float)(cy + (sy > 0 ? 1 : 0)), cell.y, org.y) - ro.y) * inv_d.y : kHuge;
        ddy = rd.y != 0.0f ? abs_(cell.y * inv_d.y) : kHuge;
    }

    while (ballot_(walking)) {
        uint32_t count = 0;
        if constexpr (COUNT) { if (walking) work.add(kCntCells); if (lane == 0) work.add(kCntWaveCells); }
        {
            // (a walking lane's indices lie inside the grid: clamped at the start, checked after every step)
            const uint32_t c = walking ? (FLATY ? (uint32_t)(cz * dx + cx) : (uint32_t)((cz * dy + cy) * dx + cx)) : 0u;
            const uint2 cw = G.cells[c];
            count = walking ? cw.x >> 16 : 0u;
            test_cell_entry<COUNT>(G, cw, count, ro, rd, a, inv_a, closest, best, work);
        }
        bool stop, inside_grid;
        if constexpr (FLATY) {
            const float t_exit = (tx < tz) ? tx : tz;
            stop = (closest <= t_exit) | (t_exit > tmax);
            const bool ax = tx <= tz;
            cx += ax ? sx : 0; cz += ax ? 0 : sz;
            tx = ax ? tx + ddx : tx; tz = ax ? tz : tz + ddz;
            inside_grid = ((uint32_t)cx < (uint32_t)dx) & ((uint32_t)cz < (uint32_t)dz);
        } else {
            const float t_exit = (tx < ty) ? ((tx < tz) ? tx : tz) : ((ty < tz) ? ty : tz);
            stop = (closest <= t_exit) | (t_exit > tmax);               // nearest hit is final, or the ray left the grid's box
            const bool ax = (tx <= ty) & (tx <= tz);
            const bool ay = !ax & (ty <= tz);
            const bool az = !ax & !ay;
            cx += ax ? sx : 0; cy += ay ? sy : 0; cz += az ? sz : 0;
            tx = ax ? tx + ddx : tx; ty = ay ? ty + ddy : ty; tz = az ? tz + ddz : tz;
            inside_grid = ((uint32_t)cx < (uint32_t)dx) & ((uint32_t)cy < (uint32_t)dy) & ((uint32_t)cz < (uint32_t)dz);
        }
        if constexpr (ANY) stop = stop | (best >= 0);
        walking = walking & !stop & inside_grid;
    }
    closest_out = closest;
    return best;
}

template <bool GRID, bool ANY, bool COUNT>
__global__ __launch_bounds__(kQueryLdsThreads, kQueryLdsMinWaves) void trace_rays_lds_kernel(RenderArgs A, const trace_f4* rays, trace_u4* hits, uint32_t n_rays)
{
    constexpr uint32_t kWaves = kQueryLdsThreads / 64u;
    const uint32_t units = n_rays / 64u + (n_rays % 64u != 0u ? 1u : 0u);
#define MIRT_LDS_SKY false
#include "mirt_lds_block_text.inc"
#undef MIRT_LDS_SKY
    const uint32_t grid_waves = gridDim.x * kWaves;
    Work<COUNT> work;
    work.clear();
#define MIRT_TRACE_SPHERES S.spheres
#define MIRT_TRACE_HIT_SPHERE (GRID ? A.spheres : S.spheres)[best]         // grid layout: one global read per hit
    for (uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6)); unit < units; unit += grid_waves) {
        const uint64_t i = (uint64_t)unit * 64u + lane;
        const bool alive = i < n_rays;
#define MIRT_TRACE_PART 1
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART

        float closest;
        int best;
        if constexpr (GRID) {
            best = A.grid_flat_y ? nearest_hit_grid_query<COUNT, ANY, true>(G, ro, rd, t_max, alive, closest, work, lane)
                                 : nearest_hit_grid_query<COUNT, ANY, false>(G, ro, rd, t_max, alive, closest, work, lane);
        } else {
#define MIRT_TRACE_PART 2
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART
        }
#define MIRT_TRACE_PART 3
#include "mirt_trace_ray_text.inc"
#undef MIRT_TRACE_PART
    }
    work.flush(A.counters, lane);
#undef MIRT_TRACE_SPHERES
#undef MIRT_TRACE_HIT_SPHERE
}

static QueryKernel trace_lds_kernel(const QueryPlan& p)
{
    return with_bools<QueryKernel>([](auto G, auto A, auto C) { return kernel_handle(trace_rays_lds_kernel<G.value, A.value, C.value>); }, p.grid, p.any, p.count);
}
