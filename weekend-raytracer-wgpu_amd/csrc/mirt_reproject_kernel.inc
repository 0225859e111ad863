// mirt_reproject_kernel.inc -- temporal reprojection by first-hit depth and id: mirt_ctx_reproject* (include/mirt.h, DESIGN.md 10.18).
// Included once by mirt_kernels.hip behind mirt_denoise_kernel.inc, exact build only: there is no fast_build:: copy.  No scene, no
// RenderArgs and no scratch.
//
//   reproject_kernel<CLAMP, RGBA8>   lane = pixel, a 64 x 4 tile per block like the denoiser's direct shape, so a wave reads 64 consecutive
//                                    records of a row: the pixel's colour (16 bytes) and guide (two 16-byte loads), then up to four taps
//                                    of the previous frame -- the guide record (two 16-byte loads, of which t and sphere are used) and one
//                                    colour record each -- at the position the pixel's first hit had under the previous camera.  With
//                                    CLAMP, eight more colour records of the neighbouring lanes, which overlap within the tile and come
//                                    from L2.  One 16-byte store, and with RGBA8 one 4-byte store.  Every load and store goes through the
//                                    queries' 4-byte-aligned vector type: the planes are the caller's.
// The rule is reproject_pixel, written once; the four instantiations differ in the clamp loop and the second store.  A tap that does
// not count is SKIPPED by a branch around its loads and sums: a record of the previous frame may be infinite or NaN, and a tap outside
// the band has no address.  The centre ray is the feature kernel's own text (mirt_centre_ray_text.inc).
//
// Every float operation below is one IEEE operation in the header's order: the file is compiled with -ffp-contract=off, and the only
// fused operations are the fma_ of the centre ray and of the hit point.

constexpr uint32_t kReprojectTileW = 64, kReprojectTileH = 4;

MIRT_DEV float reproject_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The record {r, g, b, history length} of pixel (x, compact row cy).
MIRT_DEV trace_u4 reproject_pixel(const ReprojectArgs& R, bool clamp, uint32_t x, uint32_t cy, const trace_u4* colour, const trace_u4* guides,
                                  const trace_u4* prev_colour, const trace_u4* prev_guides)
{
    const uint32_t y = R.row_begin + cy;
    CamRegs C;                                                    // what the centre ray reads, and nothing else
    C.eye = mk(R.current.eye[0], R.current.eye[1], R.current.eye[2]);
    C.hor = mk(R.current.horizontal[0], R.current.horizontal[1], R.current.horizontal[2]);
    C.ver = mk(R.current.vertical[0], R.current.vertical[1], R.current.vertical[2]);
    C.llc = mk(R.current.lower_left_corner[0], R.current.lower_left_corner[1], R.current.lower_left_corner[2]);
    C.inv_w = 1.0f / (float)R.width;
    C.inv_h = 1.0f / (float)R.height;
#include "mirt_centre_ray_text.inc"

    const uint64_t p = (uint64_t)cy * R.width + x;
    const trace_u4 g0 = guides[2u * p], g1 = guides[2u * p + 1u];
    const uint32_t id = g1.w;
    const bool hit = id != MIRT_RAY_MISS;

    // the point (a miss: the direction) in the previous camera's frame
    const f3 pe = mk(R.previous.eye[0], R.previous.eye[1], R.previous.eye[2]);
    const f3 H = mk(R.previous.horizontal[0], R.previous.horizontal[1], R.previous.horizontal[2]);
    const f3 V = mk(R.previous.vertical[0], R.previous.vertical[1], R.previous.vertical[2]);
    const f3 a = mk(R.previous.lower_left_corner[0], R.previous.lower_left_corner[1], R.previous.lower_left_corner[2]) - pe;
    const f3 at = fma3(from_bits(g0.w), rd, ro) - pe;
    const f3 rel = mk(hit ? at.x : rd.x, hit ? at.y : rd.y, hit ? at.z : rd.z);
    const f3 n = mk(H.y * V.z - H.z * V.y, H.z * V.x - H.x * V.z, H.x * V.y - H.y * V.x);
    const float s = reproject_dot(rel, n) / reproject_dot(a, n);
    const f3 q = mk(rel.x / s - a.x, rel.y / s - a.y, rel.z / s - a.z);
    const float pu = reproject_dot(q, H) / reproject_dot(H, H), pv = reproject_dot(q, V) / reproject_dot(V, V);
    const float fw = (float)R.width, fh = (float)R.height;
    const float fx = pu * fw - 0.5f, fy = (1.0f - pv) * fh - 0.5f;
    const bool ok = s > 0.0f && s < __builtin_inff() && fx > -1.0f && fx < fw && fy > -1.0f && fy < fh;
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int64_t ix = ok ? (int64_t)flx : 0, iy = ok ? (int64_t)fly : 0;        // ok: -1 <= flx < width, -1 <= fly < height
    const float wx = fx - flx, wy = fy - fly;

    float wsum = 0.0f, acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, lacc = 0.0f;
#pragma unroll
    for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = 0; dx <= 1; ++dx) {
            const int64_t qx = ix + dx, qy = iy + dy - (int64_t)R.row_begin;      // qy: the compact row
            const float bw = (dx ? wx : 1.0f - wx) * (dy ? wy : 1.0f - wy);
            if (ok && qx >= 0 && qx < (int64_t)R.width && qy >= 0 && qy < (int64_t)R.rows) {
                const uint64_t qi = (uint64_t)qy * R.width + (uint64_t)qx;
                const trace_u4 pg0 = prev_guides[2u * qi], pg1 = prev_guides[2u * qi + 1u];
                const trace_u4 pc = prev_colour[qi];
                bool counts = pg1.w == id && from_bits(pc.w) >= 1.0f;
                if (hit) counts = counts && __builtin_fabsf(from_bits(pg0.w) - s) <= R.depth_tolerance * s;
                if (counts) {
                    wsum = wsum + bw;
                    acc0 = acc0 + bw * from_bits(pc.x); acc1 = acc1 + bw * from_bits(pc.y); acc2 = acc2 + bw * from_bits(pc.z);
                    lacc = lacc + bw * from_bits(pc.w);
                }
            }
        }
    }
    const bool have = wsum >= 0.015625f;
    float h0 = acc0 / wsum, h1 = acc1 / wsum, h2 = acc2 / wsum;
    const float hlen = lacc / wsum;
    const trace_u4 cb = colour[p];
    const float c0 = from_bits(cb.x), c1 = from_bits(cb.y), c2 = from_bits(cb.z);

    if (clamp) {
        float lo0 = c0, lo1 = c1, lo2 = c2, hi0 = c0, hi1 = c1, hi2 = c2;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int64_t mx = (int64_t)x + dx, my = (int64_t)cy + dy;
                if (mx < 0 || mx >= (int64_t)R.width || my < 0 || my >= (int64_t)R.rows) continue;
                const trace_u4 mb = (dx == 0 && dy == 0) ? cb : colour[(uint64_t)my * R.width + (uint64_t)mx];
                const float m0 = from_bits(mb.x), m1 = from_bits(mb.y), m2 = from_bits(mb.z);
                lo0 = (m0 < lo0) ? m0 : lo0; lo1 = (m1 < lo1) ? m1 : lo1; lo2 = (m2 < lo2) ? m2 : lo2;
                hi0 = (m0 > hi0) ? m0 : hi0; hi1 = (m1 > hi1) ? m1 : hi1; hi2 = (m2 > hi2) ? m2 : hi2;
            }
        }
        h0 = (h0 < lo0) ? lo0 : h0; h1 = (h1 < lo1) ? lo1 : h1; h2 = (h2 < lo2) ? lo2 : h2;
        h0 = (h0 > hi0) ? hi0 : h0; h1 = (h1 > hi1) ? hi1 : h1; h2 = (h2 > hi2) ? hi2 : h2;
    }

    float nn = hlen + 1.0f;
    nn = (nn < R.max_history) ? nn : R.max_history;
    const float alpha = 1.0f / nn;
    const float r0 = h0 + alpha * (c0 - h0), r1 = h1 + alpha * (c1 - h1), r2 = h2 + alpha * (c2 - h2);
    trace_u4 o;
    o.x = have ? bits(r0) : cb.x; o.y = have ? bits(r1) : cb.y; o.z = have ? bits(r2) : cb.z;
    o.w = have ? bits(nn) : 0x3f800000u;
    return o;
}

template <bool CLAMP, bool RGBA8>
__global__ __launch_bounds__(kReprojectTileW * kReprojectTileH) void reproject_kernel(ReprojectArgs R, const trace_u4* colour, const trace_u4* guides,
                                                                                     const trace_u4* prev_colour, const trace_u4* prev_guides,
                                                                                     trace_u4* out, uint32_t* rgba8)
{
    const uint32_t lx = threadIdx.x & (kReprojectTileW - 1u), ly = threadIdx.x / kReprojectTileW;
    for (uint64_t tile = blockIdx.x; tile < R.tiles; tile += gridDim.x) {
        const uint64_t tx = (tile % R.tiles_x) * kReprojectTileW + lx, ty = (tile / R.tiles_x) * kReprojectTileH + ly;
        if (tx >= R.width || ty >= R.rows) continue;
        const uint64_t p = ty * R.width + tx;
        const trace_u4 o = reproject_pixel(R, CLAMP, (uint32_t)tx, (uint32_t)ty, colour, guides, prev_colour, prev_guides);
        out[p] = o;
        if constexpr (RGBA8)
            rgba8[p] = pack_rgba(resolve_channel((unsigned long long)to_fixed(from_bits(o.x)), 1u, R.flags),
                                 resolve_channel((unsigned long long)to_fixed(from_bits(o.y)), 1u, R.flags),
                                 resolve_channel((unsigned long long)to_fixed(from_bits(o.z)), 1u, R.flags));
    }
}

template <bool CLAMP, bool RGBA8>
static void launch_reproject_as(const ReprojectArgs& a, const void* d_colour, const void* d_guides, const void* d_prev_colour, const void* d_prev_guides,
                                void* d_out, void* d_rgba8, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)(a.tiles < (1u << 22) ? a.tiles : (1u << 22));
    hipLaunchKernelGGL((reproject_kernel<CLAMP, RGBA8>), dim3(blocks), dim3(kReprojectTileW * kReprojectTileH), 0, stream, a,
                       static_cast<const trace_u4*>(d_colour), static_cast<const trace_u4*>(d_guides), static_cast<const trace_u4*>(d_prev_colour),
                       static_cast<const trace_u4*>(d_prev_guides), static_cast<trace_u4*>(d_out), static_cast<uint32_t*>(d_rgba8));
}

// a.width, a.rows > 0; a.tiles_x and a.tiles are filled here
hipError_t launch_reproject(ReprojectArgs a, bool clamp, const void* d_colour, const void* d_guides, const void* d_prev_colour, const void* d_prev_guides,
                            void* d_out, void* d_rgba8, hipStream_t stream)
{
    a.tiles_x = (uint32_t)(((uint64_t)a.width + kReprojectTileW - 1u) / kReprojectTileW);
    a.tiles = (uint64_t)a.tiles_x * (((uint64_t)a.rows + kReprojectTileH - 1u) / kReprojectTileH);
    if (clamp) {
        if (d_rgba8) launch_reproject_as<true, true>(a, d_colour, d_guides, d_prev_colour, d_prev_guides, d_out, d_rgba8, stream);
        else launch_reproject_as<true, false>(a, d_colour, d_guides, d_prev_colour, d_prev_guides, d_out, d_rgba8, stream);
    } else {
        if (d_rgba8) launch_reproject_as<false, true>(a, d_colour, d_guides, d_prev_colour, d_prev_guides, d_out, d_rgba8, stream);
        else launch_reproject_as<false, false>(a, d_colour, d_guides, d_prev_colour, d_prev_guides, d_out, d_rgba8, stream);
    }
    return hipGetLastError();
}
