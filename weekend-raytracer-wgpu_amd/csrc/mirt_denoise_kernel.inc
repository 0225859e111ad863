// mirt_denoise_kernel.inc -- the edge-avoiding a-trous filter of mirt_ctx_denoise* (include/mirt.h, DESIGN.md 10.17).  Included once by
// mirt_kernels.hip behind mirt_radiance_lds_kernel.inc, exact build only: there is no fast_build:: copy.  No scene and no RenderArgs.
// The context's scratch holds three planes of 16 bytes per pixel, 16-byte aligned: two colour planes {c[0], c[1], c[2], 0} that the levels
// write alternately, and one guide plane {normal[0..2], sphere}.
//
//   denoise_prepare_kernel<SRC>   lane = pixel.  Reads the pixel's three sums (SRC 0: the accumulation buffer, n the launch's; SRC 1: a
//                                 MirtAdaptPixel, two 16-byte loads and the count) and the caller's guide as two 16-byte loads through the
//                                 4-byte-aligned vector type of the queries; writes two 16-byte stores: {m / den, 0} and {normal, sphere}.
//   denoise_atrous_kernel<LAST>   the DIRECT shape: lane = pixel, a 64 x 4 tile per block, so a wave reads 64 consecutive records of a row per
//                                 tap: 1 KB per load, served by L2 and the Infinity Cache.  One text serves every level; the level's step,
//                                 1 / sg^2 and the two exponents are arguments.  A tap is two 16-byte loads.  A tap outside the band is
//                                 loaded from a clamped address with kernel weight 0: its products are +0 or -0 and every sum starts from
//                                 +0, so the bits are those of skipping it.  LAST 0 stores the level's {c', 0}; LAST 1 and 2 are the final
//                                 level's epilogues: c' x den from the caller's guides again, to RGBA8 through to_fixed and
//                                 resolve_channel, or to {r, g, b, 1.0f}.
//   denoise_atrous_staged_kernel<LAST>   the STAGED shape: a 256-thread block owns a 32 x 8 tile of the pixels of one residue class modulo
//                                 the step and stages the 36 x 12 records its taps touch in LDS, 13.8 KB at every level; the same tap
//                                 arithmetic (denoise_tap) on records read from there, the same epilogues.
// Which shape a level runs is the host's choice by the level (mirt_api.hip, kDenoiseStagedLevels; DESIGN.md 10.17 has the measurement):
// the bytes are the same.  The tap weight keeps its branches: written with selects alone the kernels take 185 - 248 VGPRs (2 waves per
// SIMD instead of 3) and a level 30 % longer.
//
// Every float operation below is one IEEE operation in the header's order: the file is compiled with -ffp-contract=off and spells no fma.

typedef float denoise_f4 __attribute__((ext_vector_type(4)));         // a plane's record, 16-byte aligned (the scratch is the context's own)
typedef uint32_t denoise_u4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kDenoiseTileW = 64, kDenoiseTileH = 4;             // denoise_atrous_kernel: pixels per block, one wave per row of the tile

// what a level needs beside its planes
struct DenoiseLevel {
    uint32_t width, rows;          // of the band
    uint32_t step;                 // 1 << level
    uint32_t normal_log2;
    uint32_t colour;               // sigma_colour != 0
    float    inv;                  // 1 / (sigma_colour 2^-level)^2, computed on the host
    uint32_t flags;                // MIRT_FLAG_NO_TONEMAP | MIRT_FLAG_NO_SRGB (LAST 1)
    uint32_t tiles_x, tiles_y;     // direct: ceil(width / kDenoiseTileW), ceil(rows / kDenoiseTileH); staged: those of ONE residue class
    uint64_t tiles;                // direct: tiles_x * tiles_y; staged: step^2 classes of them
};

MIRT_DEV float denoise_mean(unsigned long long sum, uint32_t n)
{
    const float m = (float)((double)sum / ((double)n * 1048576.0));
    return (n != 0u) ? m : 0.0f;
}

MIRT_DEV float denoise_den(float albedo, bool hit) { return (hit && albedo >= 0.015625f && albedo <= 64.0f) ? albedo : 1.0f; }

template <int SRC>
__global__ __launch_bounds__(256) void denoise_prepare_kernel(const void* src, uint32_t n_samples, const trace_u4* guides, uint64_t n_pixels,
                                                              denoise_f4* colour, denoise_u4* guide)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long s0, s1, s2;
        uint32_t n;
        if constexpr (SRC == 0) {
            const unsigned long long* a = static_cast<const unsigned long long*>(src) + 3u * i;
            s0 = a[0]; s1 = a[1]; s2 = a[2];
            n = n_samples;
        } else {
            const adapt_u4* r = static_cast<const adapt_u4*>(src) + 4u * i;
            const adapt_u4 q0 = r[0], q1 = r[1], q3 = r[3];
            s0 = adapt_u64(q0.x, q0.y); s1 = adapt_u64(q0.z, q0.w); s2 = adapt_u64(q1.x, q1.y);
            n = q3.x;
        }
        const trace_u4 g0 = guides[2u * i], g1 = guides[2u * i + 1u];
        const bool hit = g1.w != MIRT_RAY_MISS;
        denoise_f4 c;
        c.x = denoise_mean(s0, n) / denoise_den(from_bits(g0.x), hit);
        c.y = denoise_mean(s1, n) / denoise_den(from_bits(g0.y), hit);
        c.z = denoise_mean(s2, n) / denoise_den(from_bits(g0.z), hit);
        c.w = 0.0f;
        colour[i] = c;
        denoise_u4 g;
        g.x = g1.x; g.y = g1.y; g.z = g1.z; g.w = g1.w;
        guide[i] = g;
    }
}

// One tap that is not the centre: its weight from the two records, then the three sums in the header's order.  kern is 0 for a tap
// outside the band (any finite record may stand in for it then).
struct DenoiseSums { float wsum, a0, a1, a2; };

MIRT_DEV void denoise_tap(const DenoiseLevel& L, const denoise_f4 cp, const denoise_u4 gp, const denoise_f4 cq, const denoise_u4 gq, float kern, DenoiseSums& S)
{
    float wg;
    if (gq.w != gp.w) wg = 0.0f;
    else if (gp.w == MIRT_RAY_MISS) wg = 1.0f;
    else {
        float t = (from_bits(gp.x) * from_bits(gq.x) + from_bits(gp.y) * from_bits(gq.y)) + from_bits(gp.z) * from_bits(gq.z);
        t = (t > 0.0f) ? ((t < 1.0f) ? t : 1.0f) : 0.0f;
        for (uint32_t k = 0; k < L.normal_log2; ++k) t = t * t;
        wg = t;
    }
    float wc = 1.0f;
    if (L.colour) {
        const float d0 = cp.x - cq.x, d1 = cp.y - cq.y, d2 = cp.z - cq.z;
        const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
        wc = exp_(-(dd * L.inv));
    }
    const float w = (kern * wg) * wc;
    S.wsum = S.wsum + w;
    S.a0 = S.a0 + w * cq.x; S.a1 = S.a1 + w * cq.y; S.a2 = S.a2 + w * cq.z;
}

MIRT_DEV void denoise_centre(const denoise_f4 cp, DenoiseSums& S)
{
    S.wsum = S.wsum + 36.0f;
    S.a0 = S.a0 + 36.0f * cp.x; S.a1 = S.a1 + 36.0f * cp.y; S.a2 = S.a2 + 36.0f * cp.z;
}

// A level's result for pixel p: the next plane's record, or the final level's epilogue.
template <int LAST>
MIRT_DEV void denoise_store(const DenoiseLevel& L, uint64_t p, const DenoiseSums& S, bool hit, denoise_f4* cout, const trace_u4* guides, void* out)
{
    const float r0 = S.a0 / S.wsum, r1 = S.a1 / S.wsum, r2 = S.a2 / S.wsum;
    if constexpr (LAST == 0) {
        denoise_f4 c;
        c.x = r0; c.y = r1; c.z = r2; c.w = 0.0f;
        cout[p] = c;
    } else {
        const trace_u4 g0 = guides[2u * p];
        const float f0 = r0 * denoise_den(from_bits(g0.x), hit), f1 = r1 * denoise_den(from_bits(g0.y), hit), f2 = r2 * denoise_den(from_bits(g0.z), hit);
        if constexpr (LAST == 1) {
            static_cast<uint32_t*>(out)[p] = pack_rgba(resolve_channel((unsigned long long)to_fixed(f0), 1u, L.flags),
                                                       resolve_channel((unsigned long long)to_fixed(f1), 1u, L.flags),
                                                       resolve_channel((unsigned long long)to_fixed(f2), 1u, L.flags));
        } else {
            trace_u4 o;
            o.x = bits(f0); o.y = bits(f1); o.z = bits(f2); o.w = 0x3f800000u;
            static_cast<trace_u4*>(out)[p] = o;
        }
    }
}

template <int LAST>
__global__ __launch_bounds__(kDenoiseTileW * kDenoiseTileH) void denoise_atrous_kernel(DenoiseLevel L, const denoise_f4* cin, const denoise_u4* gin,
                                                                                      denoise_f4* cout, const trace_u4* guides, void* out)
{
    const uint32_t lx = threadIdx.x & (kDenoiseTileW - 1u), ly = threadIdx.x / kDenoiseTileW;
    for (uint64_t tile = blockIdx.x; tile < L.tiles; tile += gridDim.x) {
        const uint64_t x = (tile % L.tiles_x) * kDenoiseTileW + lx, y = (tile / L.tiles_x) * kDenoiseTileH + ly;
        if (x >= L.width || y >= L.rows) continue;
        const uint64_t p = y * L.width + x;
        const denoise_f4 cp = cin[p];
        const denoise_u4 gp = gin[p];
        DenoiseSums S{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                constexpr float b[5] = { 1.0f, 4.0f, 6.0f, 4.0f, 1.0f };
                if (dx == 0 && dy == 0) { denoise_centre(cp, S); continue; }
                const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)L.step, qy = (int64_t)y + (int64_t)dy * (int64_t)L.step;
                const bool in = qx >= 0 && qx < (int64_t)L.width && qy >= 0 && qy < (int64_t)L.rows;
                const uint64_t q = in ? (uint64_t)qy * L.width + (uint64_t)qx : p;          // outside: any valid record, at weight 0
                denoise_tap(L, cp, gp, cin[q], gin[q], in ? b[dx + 2] * b[dy + 2] : 0.0f, S);
            }
        }
        denoise_store<LAST>(L, p, S, gp.w != MIRT_RAY_MISS, cout, guides, out);
    }
}

// The staged shape: a block owns a kDenoiseStageW x kDenoiseStageH tile of the pixels of ONE residue class modulo the step -- x = rx + step i,
// y = ry + step j --, whose taps are its neighbours in class coordinates.  It stages the (W + 4) x (H + 4) records its taps touch in LDS
// (13.8 KB at every level; records outside the band as zeros, which the taps weigh with 0) and reads every tap from there.
constexpr uint32_t kDenoiseStageW = 32, kDenoiseStageH = 8;
constexpr uint32_t kDenoiseHaloW = kDenoiseStageW + 4u, kDenoiseHaloH = kDenoiseStageH + 4u;

template <int LAST>
__global__ __launch_bounds__(kDenoiseStageW * kDenoiseStageH) void denoise_atrous_staged_kernel(DenoiseLevel L, const denoise_f4* cin, const denoise_u4* gin,
                                                                                               denoise_f4* cout, const trace_u4* guides, void* out)
{
    __shared__ denoise_f4 sc[kDenoiseHaloW * kDenoiseHaloH];
    __shared__ denoise_u4 sg[kDenoiseHaloW * kDenoiseHaloH];
    const uint32_t li = threadIdx.x & (kDenoiseStageW - 1u), lj = threadIdx.x / kDenoiseStageW;
    const uint64_t s = L.step, per_class = (uint64_t)L.tiles_x * L.tiles_y;           // tiles_x, tiles_y: of one class
    for (uint64_t tile = blockIdx.x; tile < L.tiles; tile += gridDim.x) {
        const uint64_t cls = tile / per_class, t = tile % per_class;
        const uint64_t rx = cls % s, ry = cls / s;
        const int64_t i0 = (int64_t)((t % L.tiles_x) * kDenoiseStageW), j0 = (int64_t)((t / L.tiles_x) * kDenoiseStageH);
        for (uint32_t k = threadIdx.x; k < kDenoiseHaloW * kDenoiseHaloH; k += kDenoiseStageW * kDenoiseStageH) {
            const int64_t ci = i0 + (int64_t)(k % kDenoiseHaloW) - 2, cj = j0 + (int64_t)(k / kDenoiseHaloW) - 2;
            const int64_t x = (int64_t)rx + (int64_t)s * ci, y = (int64_t)ry + (int64_t)s * cj;
            denoise_f4 c = { 0.0f, 0.0f, 0.0f, 0.0f };
            denoise_u4 g = { 0u, 0u, 0u, 0u };
            if (ci >= 0 && cj >= 0 && x < (int64_t)L.width && y < (int64_t)L.rows) {
                const uint64_t q = (uint64_t)y * L.width + (uint64_t)x;
                c = cin[q];
                g = gin[q];
            }
            sc[k] = c;
            sg[k] = g;
        }
        __syncthreads();
        const uint64_t x = rx + s * ((uint64_t)i0 + li), y = ry + s * ((uint64_t)j0 + lj);
        if (x < L.width && y < L.rows) {
            const uint32_t at = (lj + 2u) * kDenoiseHaloW + li + 2u;
            const denoise_f4 cp = sc[at];
            const denoise_u4 gp = sg[at];
            DenoiseSums S{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    constexpr float b[5] = { 1.0f, 4.0f, 6.0f, 4.0f, 1.0f };
                    if (dx == 0 && dy == 0) { denoise_centre(cp, S); continue; }
                    const int64_t qx = (int64_t)x + (int64_t)dx * (int64_t)s, qy = (int64_t)y + (int64_t)dy * (int64_t)s;
                    const bool in = qx >= 0 && qx < (int64_t)L.width && qy >= 0 && qy < (int64_t)L.rows;
                    const uint32_t q = (uint32_t)((int)at + dy * (int)kDenoiseHaloW + dx);
                    denoise_tap(L, cp, gp, sc[q], sg[q], in ? b[dx + 2] * b[dy + 2] : 0.0f, S);
                }
            }
            denoise_store<LAST>(L, y * L.width + x, S, gp.w != MIRT_RAY_MISS, cout, guides, out);
        }
        __syncthreads();                        // the next tile overwrites the staged records
    }
}

template <int LAST>
static void launch_denoise_level(bool staged, const DenoiseLevel& L, const denoise_f4* cin, const denoise_u4* guide, denoise_f4* cout, const trace_u4* guides,
                                 void* d_out, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)(L.tiles < (1u << 22) ? L.tiles : (1u << 22));
    if (staged) hipLaunchKernelGGL(denoise_atrous_staged_kernel<LAST>, dim3(blocks), dim3(kDenoiseStageW * kDenoiseStageH), 0, stream, L, cin, guide, cout, guides, d_out);
    else hipLaunchKernelGGL(denoise_atrous_kernel<LAST>, dim3(blocks), dim3(kDenoiseTileW * kDenoiseTileH), 0, stream, L, cin, guide, cout, guides, d_out);
}

// The kernels of one call on `stream`: prepare, then `levels` a-trous launches of which the last carries the epilogue.  d_scratch holds
// three planes of n_pixels x 16 bytes; inv[i] is level i's 1 / sg^2; bit i of staged_levels: level i runs the staged shape.
hipError_t launch_denoise(uint32_t source, const void* d_src, uint32_t n_samples, const void* d_guides, uint32_t width, uint32_t rows, uint32_t levels,
                          uint32_t normal_log2, bool colour, const float* inv, bool f32_out, uint32_t flags, uint32_t staged_levels, void* d_scratch, void* d_out,
                          hipStream_t stream)
{
    const uint64_t n_pixels = (uint64_t)width * rows;
    denoise_f4* plane[2] = { static_cast<denoise_f4*>(d_scratch), static_cast<denoise_f4*>(d_scratch) + n_pixels };
    denoise_u4* guide = reinterpret_cast<denoise_u4*>(plane[1] + n_pixels);
    const trace_u4* guides = static_cast<const trace_u4*>(d_guides);
    uint64_t pb = (n_pixels + 255u) / 256u;
    if (pb > (1u << 20)) pb = 1u << 20;
    if (source == MIRT_DENOISE_SRC_ACCUM)
        hipLaunchKernelGGL(denoise_prepare_kernel<0>, dim3((uint32_t)pb), dim3(256), 0, stream, d_src, n_samples, guides, n_pixels, plane[0], guide);
    else
        hipLaunchKernelGGL(denoise_prepare_kernel<1>, dim3((uint32_t)pb), dim3(256), 0, stream, d_src, n_samples, guides, n_pixels, plane[0], guide);
    DenoiseLevel L{};
    L.width = width; L.rows = rows; L.normal_log2 = normal_log2; L.colour = colour ? 1u : 0u; L.flags = flags;
    for (uint32_t i = 0; i < levels; ++i) {
        const bool staged = ((staged_levels >> i) & 1u) != 0u;
        L.step = 1u << i;
        L.inv = inv[i];
        if (staged) {
            const uint64_t cw = ((uint64_t)width + L.step - 1u) / L.step, ch = ((uint64_t)rows + L.step - 1u) / L.step;      // of the widest class
            L.tiles_x = (uint32_t)((cw + kDenoiseStageW - 1u) / kDenoiseStageW);
            L.tiles_y = (uint32_t)((ch + kDenoiseStageH - 1u) / kDenoiseStageH);
            L.tiles = (uint64_t)L.step * L.step * L.tiles_x * L.tiles_y;
        } else {
            L.tiles_x = (uint32_t)(((uint64_t)width + kDenoiseTileW - 1u) / kDenoiseTileW);
            L.tiles_y = (uint32_t)(((uint64_t)rows + kDenoiseTileH - 1u) / kDenoiseTileH);
            L.tiles = (uint64_t)L.tiles_x * L.tiles_y;
        }
        const denoise_f4* cin = plane[i & 1u];
        denoise_f4* cout = plane[(i + 1u) & 1u];
        if (i + 1u < levels) launch_denoise_level<0>(staged, L, cin, guide, cout, guides, d_out, stream);
        else if (!f32_out)   launch_denoise_level<1>(staged, L, cin, guide, cout, guides, d_out, stream);
        else                 launch_denoise_level<2>(staged, L, cin, guide, cout, guides, d_out, stream);
    }
    return hipGetLastError();
}
