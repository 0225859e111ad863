// mirt_pool_kernel.inc -- the text of the pooled path-traced kernel.  mirt_kernels.hip includes it twice, and twice more with
// MIRT_POOL_KERNEL_FRAME = true for the progressive-frame builds (render_pt_pool_frame_kernel, render_pt_pool_tile_frame_kernel):
//   MIRT_POOL_KERNEL_NAME = render_pt_pool_kernel,      MIRT_POOL_KERNEL_TILE = false   (the default build)
//   MIRT_POOL_KERNEL_NAME = render_pt_pool_tile_kernel, MIRT_POOL_KERNEL_TILE = true    (MIRT_FLAG_TEXEL_TILES: flat scenes with an
//       image texture; a texel window per wave behind its pool)
// Two kernels from one text instead of one more template parameter or a shared body function: the default kernel keeps its
// name in every profile, and its code is compiled exactly as before (routing it through an inlined body function cost 7.8 %
// on config 3: 70 -> 80 VGPRs and a different schedule).
template <uint32_t THREADS, uint32_t SLOTS, uint32_t MINW, bool COUNT, bool HOSEK, uint32_t NQ = 5, bool GRID = false, bool FLATY = false>
__global__ __launch_bounds__(THREADS, MINW) void MIRT_POOL_KERNEL_NAME(RenderArgs A)
{
    constexpr bool TILE = MIRT_POOL_KERNEL_TILE;
    constexpr bool FRAME = MIRT_POOL_KERNEL_FRAME;         // the progressive-frame build: see the strip's epilogue
    using Lay = WavePoolLayout<SLOTS, NQ, GRID, TILE>;
    static_assert(!(GRID && TILE), "the tile build exists for flat scenes");
    static_assert(GRID || !FLATY, "FLATY: a grid one cell high");
    constexpr uint32_t OP_GEN = NQ, OP_WALK = NQ + 1, kNumOps = Lay::kQueues;
    static_assert(NQ >= 1 && NQ < kMaxQueues, "scatter queues");
    constexpr uint32_t RING = Lay::kRing;
    static_assert(SLOTS >= 64 && SLOTS <= 256 && SLOTS % 8 == 0, "slot ids are 8 bit");
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, !GRID>(A, smem, HOSEK);
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t scene_bytes = (uint32_t)scene_lds_bytes_dev(A.n_spheres, A.n_mats, HOSEK, !GRID);
    GridLds G{};
    if constexpr (GRID) { G = stage_grid(A, smem + scene_bytes); scene_bytes += A.grid_bytes; }
    constexpr bool HOLD_CAM = !GRID && !HOSEK && !TILE && !COUNT && MINW == 6;        // see CamHeld: the default geometry has the registers
    CamHeld CH{};
    if constexpr (HOLD_CAM) CH = hold_camera(S);
    GridConsts GC{};                                       // grid builds: the header's fields and up to four big-sphere records, in registers
    if constexpr (GRID) GC = load_grid_consts(G);
    unsigned char* pool = smem + scene_bytes + wave * Lay::kBytes;
    uint4* const L_state = reinterpret_cast<uint4*>(pool + Lay::kOffState);
    unsigned long long* const L_acc = reinterpret_cast<unsigned long long*>(pool + Lay::kOffAcc);
    unsigned char* const L_ring = pool + Lay::kOffRing;
    unsigned short* const L_cell = reinterpret_cast<unsigned short*>(pool + Lay::kOffCell);
    unsigned short* const L_cand = reinterpret_cast<unsigned short*>(pool + Lay::kOffCand);             // GRID: ids [kMaxCand], then the count
    uint32_t* const L_cand_n = reinterpret_cast<uint32_t*>(pool + Lay::kOffCand + 2 * kMaxCand);
    // PIXREC: the strip's pixel records in the spare fourth word of the slots' third vector (see WavePoolLayout's notes); word k of pixel
    // p's record lies 144 p + 48 k bytes behind slot 0's (a 24-bit multiply-add: p < 16)
    constexpr bool PIXREC = MIRT_GEN_PIXEL_RECORDS != 0 && !GRID;
    static_assert(!PIXREC || SLOTS >= 3 * kStripPixels, "three slots per pixel of a strip");
    unsigned char* const L_pixw = pool + Lay::kOffState + 44;
    const auto pix_word = [L_pixw](uint32_t p, uint32_t k) -> uint32_t& { return *reinterpret_cast<uint32_t*>(L_pixw + __umul24(p, 144u) + 48u * k); };
    TexelTile tile{ reinterpret_cast<uint32_t*>(pool + Lay::kOffTile), reinterpret_cast<float*>(pool + Lay::kOffTile + 16), 0u, 0u, 0u, 0u, 0u, 0u };
    TexelTile* const T = TILE ? &tile : nullptr;

    Work<COUNT> work;
    work.clear();
    Stamps stamps;                                     // diagnosis builds only (MIRT_DIAG_STAMPS); empty otherwise
    stamps.start();

    for (uint32_t strip = first_unit(); strip < A.n_units; strip = next_unit_any(A, lane)) {
        // which level does this unit belong to?  (wave-uniform scalar code, once per strip)
        const RenderArgs& AP = per_strip_args();         // the arguments this prologue needs, loaded here and now
        uint32_t lvl = 0;
#pragma unroll
        for (uint32_t l = 1; l < kStripLevels; ++l) lvl = (strip >= AP.lvl_unit[l]) ? l : lvl;
        uint32_t unit0 = AP.lvl_unit[0], pix0 = AP.lvl_pix[0], pix_end = AP.lvl_pix[1];
#pragma unroll
        for (uint32_t l = 1; l < kStripLevels; ++l)
            if (lvl == l) { unit0 = AP.lvl_unit[l]; pix0 = AP.lvl_pix[l]; pix_end = AP.lvl_pix[l + 1]; }
        const uint32_t width_log2 = 4u - lvl;              // 16, 8, 4, 2, 1 pixels
        const uint32_t base_pix = pix0 + ((strip - unit0) << width_log2);
        const uint32_t want_pixels = 1u << width_log2;
        const uint32_t strip_pixels = (pix_end - base_pix < want_pixels) ? (pix_end - base_pix) : want_pixels;
        const uint32_t total_items = strip_pixels * AP.spp;
        // scalar (per-strip) pixel addressing: one division here instead of two per work item
        const uint32_t base_ci = base_pix / AP.width;
        const uint32_t base_x = base_pix - base_ci * AP.width;
        const bool wide = AP.width >= kStripPixels;           // a strip then spans at most two rows
        const uint32_t row0 = abs_row(AP, base_ci);
        const uint32_t row1 = (base_ci + 1 < AP.out_rows) ? abs_row(AP, base_ci + 1) : row0;

        // all slots start in the OP_GEN queue
        for (uint32_t s = lane; s < SLOTS; s += 64) { L_ring[OP_GEN * RING + s] = (unsigned char)s; L_state[s * 3].w = 0u; }
        if (lane < kStripPixels * 3) L_acc[lane] = 0ull;
        if constexpr (PIXREC) {
            // what a GEN step needs of its pixel, once per strip instead of once per sample: pixel `lane` of the strip -> (x, y) -- the strip
            // starts at (base_x, row0) and may wrap into following rows -- as floats, and the pixel's part of the seed (generate_primary)
            if (lane < strip_pixels) {
                uint32_t x = base_x + lane, y = row0;
                if (wide) { if (x >= AP.width) { x -= AP.width; y = row1; } }
                else { const uint32_t pi = base_pix + lane; const uint32_t ci = pi / AP.width; x = pi - ci * AP.width; y = abs_row(AP, ci); }
                pix_word(lane, 0) = bits((float)x); pix_word(lane, 1) = bits((float)y); pix_word(lane, 2) = (x + y * AP.width) ^ AP.seed_mix;
            }
        }
        if constexpr (TILE) tile.reset(lane);              // the strip's first image fetch places the window
        if constexpr (GRID) {                              // the spheres this strip's camera rays can touch (strip_candidates)
            uint32_t n_cand = kNoCand;
            if (AP.strip_cand != 0u && wide && base_x + strip_pixels <= AP.width)
                n_cand = strip_candidates(AP, S, base_x, strip_pixels, row0, L_cand, lane);
            if (lane == 0) *L_cand_n = n_cand;
#define MIRT_PROBE_SITE 6           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE
        }
        // Each queue is a STACK of slot ids (order of service is free: the image does not depend on it), so a
        // queue is described by its depth alone -- NQ + 1 SGPRs, no heads, no index wrap.
        uint32_t tail[kNumOps];                            // wave-uniform (SGPRs)
#pragma unroll
        for (uint32_t k = 0; k < kNumOps; ++k) tail[k] = (k == OP_GEN) ? SLOTS : 0u;
        uint32_t next_item = 0;

        // Loop-carried path state of the lanes (registers).  A normal step loads it from the wave's pool (pick a queue,
        // pop slot ids, gather); a FAST-FORWARD step inherits it from the step before: when every lane of a step moves
        // on to the SAME routine (coherent primary rays all hitting the ground, sky pixels going straight back to OP_GEN:
        // 43 % of all steps on config 3), storing the paths, pushing, picking, popping and gathering them again would
        // only move the same 64 paths through LDS, so the wave runs that routine on them right away.  The order in
        // which paths are served is free (exact integer accumulation), so the image cannot change.
        bool ff = false;                                   // wave-uniform
        uint32_t my_k = 0, my_n = 0;                       // wave-uniform: routine of this step, number of paths
        uint32_t slot = 0, pix = 0, bounce = 0, missf = 0;
        int best = 0;
        float walk_closest = kMaxT;                        // GRID: state of a path whose grid walk is cut (OP_WALK)
        uint32_t walk_cell = 0;
        f3 ro = mk(0, 0, 0), rd = mk(0, 0, 0), thr = mk(0, 0, 0);
        Rng rng;
        rng.state = 0;

        for (;;) {
            stamps.mark(6);                            // the previous step's tail: classification, fast-forward test, store, push
            if (!ff) {
                // ---- pick the deepest queue: max over keys depth << 3 | (7 - op); ties go to the lower op ----
                const uint32_t key = deepest_key<0>(tail);
                const uint32_t depth = key >> 3;
                if (depth == 0) break;                     // every queue empty: strip finished
                my_k = 7u - (key & 7u);
                my_n = (depth > 64u) ? 64u : depth;
                const uint32_t my_begin = depth - my_n;    // the top my_n entries
#pragma unroll
                for (uint32_t k = 0; k < kNumOps; ++k) {
                    tail[k] -= (my_k == k) ? my_n : 0u;
                }

                // ---- pop + gather ----
                const bool has0 = lane < my_n;
                slot = has0 ? (uint32_t)L_ring[my_k * RING + my_begin + lane] : 0u;
                const uint4 q0 = L_state[slot * 3 + 0], q1 = L_state[slot * 3 + 1], q2 = L_state[slot * 3 + 2];
                const uint32_t fl = q0.w;
                ro = mk(from_bits(q0.x), from_bits(q0.y), from_bits(q0.z));      // the hit point for scatter steps
                rd = mk(from_bits(q1.x), from_bits(q1.y), from_bits(q1.z));
                best = has0 ? (int)(fl & 0xfffu) : 0;
                if constexpr (GRID) {
                    if (my_k == OP_WALK) {                 // a cut walk: nearest hit so far (none: bit 25) and the cell to resume in
                        best = (fl >> 25) & 1u ? best : -1;
                        walk_closest = from_bits(q2.w);
                        walk_cell = L_cell[slot];
                    }
                }
                thr = mk(from_bits(q2.x), from_bits(q2.y), from_bits(q2.z));
                rng.state = q1.w;
                pix = (fl >> 12) & 0xfu;
                bounce = (fl >> 16) & 0xffu;
                missf = (fl >> 24) & 1u;
            }
            const bool has = lane < my_n;
            bool alive = has;
            if constexpr (COUNT) { if (lane == 0) work.add(kCntWaveIters); }
#define MIRT_PROBE_SITE 4           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE

            stamps.mark(0);                            // pick + pop + gather
            if (my_k == OP_GEN) {
                // finish the previous path of this slot ...
                if (has && missf) {
                    work.add(kCntSky);
                    const f3 c = sky_color<HOSEK>(S, rd);
                    atomicAdd(&L_acc[pix * 3 + 0], (unsigned long long)to_fixed(thr.x * c.x));
                    atomicAdd(&L_acc[pix * 3 + 1], (unsigned long long)to_fixed(thr.y * c.y));
                    atomicAdd(&L_acc[pix * 3 + 2], (unsigned long long)to_fixed(thr.z * c.z));
                }
                // ... and start the next work item in it
                const uint32_t item = next_item + lane;
                next_item += my_n;
                alive = has && item < total_items;
                uint32_t sample;
                if (strip_pixels == want_pixels) { sample = item >> width_log2; pix = item & (want_pixels - 1u); }
                else { sample = item / strip_pixels; pix = item - sample * strip_pixels; }      // ragged last strip
                // camera constants are (re)read from LDS here, 6 broadcast ds_read_b128 per GEN step, instead of
                // living in 21 VGPRs across the whole kernel: the kernel then fits 6 waves per SIMD
                if constexpr (PIXREC) {
                    // the pixel's record, read with the camera rows: the same wait
                    const float fx = from_bits(pix_word(pix, 0)), fy = from_bits(pix_word(pix, 1));
                    const uint32_t pixel_key = pix_word(pix, 2);
                    const CamRegs C = HOLD_CAM ? load_camera(S, A, CH) : load_camera(S, A);
                    generate_primary(C, fx, fy, pixel_key, A.sample_begin + sample, rng, ro, rd);
                } else {
                    // pixel -> (x, y): the strip starts at (base_x, row0) and may wrap into following rows
                    uint32_t x = base_x + pix, y = row0;
                    if (wide) { if (x >= A.width) { x -= A.width; y = row1; } }
                    else { const uint32_t pi = base_pix + pix; const uint32_t ci = pi / A.width; x = pi - ci * A.width; y = abs_row(A, ci); }
                    const CamRegs C = HOLD_CAM ? load_camera(S, A, CH) : load_camera(S, A);
                    generate_primary(A, C, x, y, A.sample_begin + sample, rng, ro, rd);
                }
                thr = mk(1, 1, 1);
                bounce = 0;
            } else if (GRID && my_k == OP_WALK) {
                // nothing to shade: the tail below resumes these paths' grid walks
            } else {
                // sphereIntersection wgsl:431-440, then ONE scatter routine for the whole wave
                const f3 hp = ro;                          // computed by the tail of the step that found the hit
                f3 ndir = rd, att = mk(1, 1, 1);
                // lanes without a slot run the routine too, on slot 0's (valid) state: their results are never
                // stored, and leaving them in saves an exec-mask region around every routine
                if constexpr (GRID) {
                    // Grid builds (many-sphere scenes) keep ONE scatter queue and switch on the material per lane: there the
                    // trace -- grid set-up, big spheres, cell walk -- is 70 % of a step and shading the smaller part, so fuller
                    // steps (3 queues share the slots instead of 5) are worth more than undivided routines: -7 % on RTIOW.
                    // They keep no material table in LDS: a hit reads 1/r and its material from the sphere's ShadeRec in global
                    // memory / L1 -- two independent 16-byte loads (round 3: four; the texture cache serves 64 different lines per
                    // wave-load, one per cycle, and was a third busy with them) that shade_grid_hit needs only after its draws.
                    const float4* rec = reinterpret_cast<const float4*>(&A.shade[best]);
                    const float4 ra = rec[0], t0 = rec[1];           // {1/r, x, 1/x, flags}, first texture: two loads in flight ...
                    const uint32_t rid = G.ops[best];                // ... while the routine id and the centre come from LDS
                    const float4 c4 = G.recs[best];
                    { const Scattered sc = shade_grid_hit<COUNT>(A, rid, rec, ra, t0, mk(c4.x, c4.y, c4.z), has, rd, hp, rng, work); ndir = sc.dir; att = sc.att; }
                } else {
                const PreparedSphere sp = S.spheres[best];
                const f3 hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
                const PreparedMaterial* m = &S.pmats[has ? sp.material_idx : 0u];
                uint32_t routine = A.queue_routine[0];     // wave-uniform dispatch
#pragma unroll
                for (uint32_t k = 1; k < NQ; ++k) routine = (my_k == k) ? A.queue_routine[k] : routine;
                if (routine == RT_LAMBERTIAN) {
                    if (has) work.add(kCntScatter0);
                    shade_lambertian(A, m, hn, rng, ndir, att, T);
                } else if (routine == RT_METAL) {
                    if (has) work.add(kCntScatter1);
                    shade_metal(A, m, rd, hn, rng, ndir, att, T);
                } else if (routine == RT_DIELECTRIC) {
                    if (has) work.add(kCntScatter2);
                    shade_dielectric(m, rd, hn, rng, ndir, att);
                } else if (routine == RT_CHECKER) {
                    if (has) work.add(kCntScatter3);
                    shade_checkerboard(A, m, hp, hn, rng, ndir, att, T);
                } else {
                    if (has) work.add(kCntScatter4);
                    shade_missing(hn, rng, ndir, att);
                }
#define MIRT_PROBE_SITE 1           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE
                }
                if constexpr (TILE) tile.refresh();
                if constexpr (TILE && COUNT) {            // image-texel fetches of the paths this step shaded: camera-ray hits / later bounces
                    if (has) { work.add(bounce == 0u ? kCntTexelsPrimary : kCntTexelsLater, tile.fetched);
                               work.add(bounce == 0u ? kCntTileHitsPrimary : kCntTileHitsLater, tile.from_tile); }
                    tile.fetched = 0u; tile.from_tile = 0u;
                }
                ro = hp;
                rd = ndir;
                thr = thr * att;
                bounce += 1;
            }

#define MIRT_PROBE_SITE 2           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE
            if (my_k == OP_GEN) stamps.mark(1); else stamps.mark(2);       // generate / scatter (2 also takes the empty front of a resumed walk)
            // common tail: bounce limit (wgsl:130), nearest hit, classification
            const bool resume = GRID && my_k == OP_WALK;   // wave-uniform
            const bool trace = alive && (resume || bounce < A.num_bounces);
            if constexpr (COUNT) { if (trace && !resume) work.add(kCntLaneIters); }
            float closest;
            int nb;
            bool cut = false;                              // GRID: the walk used up its cell budget: continue in an OP_WALK step
            if constexpr (GRID) {
                closest = walk_closest;
                nb = best;
                uint32_t n_cand = kNoCand;
                if (my_k == OP_GEN) n_cand = __builtin_amdgcn_readfirstlane(*L_cand_n);
                if (n_cand != kNoCand) {
                    // camera rays of a strip with a candidate list: a flat scan of the list (ids and records are broadcast reads)
                    closest = kMaxT;
                    nb = -1;
                    if (trace) work.add(kCntRays);
                    const float a = dot(rd, rd);
                    const float inv_a = rcp_(a);
                    // ids: eight per 16-byte broadcast read; records: four in flight per LDS round trip (the list is 4 long on average)
                    const uint4* idq = reinterpret_cast<const uint4*>(L_cand);
                    for (uint32_t j0 = 0; j0 < n_cand; j0 += 8u) {
                        const uint4 q = idq[j0 >> 3];
                        const uint32_t w4[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
                        for (uint32_t h = 0; h < 2u; ++h) {
                            if (j0 + 4u * h >= n_cand) break;                  // wave-uniform
                            const uint32_t i0 = w4[2 * h] & 0xffffu, i1 = w4[2 * h] >> 16, i2 = w4[2 * h + 1] & 0xffffu, i3 = w4[2 * h + 1] >> 16;
                            const uint32_t left = n_cand - (j0 + 4u * h);      // >= 1; ids beyond the list are stale but valid sphere ids or 0
                            const float4 r0 = G.recs[i0], r1 = G.recs[left > 1u ? i1 : 0u], r2 = G.recs[left > 2u ? i2 : 0u], r3 = G.recs[left > 3u ? i3 : 0u];
                            test_sphere<COUNT>(r0, i0, ro, rd, a, inv_a, trace, closest, nb, work);
                            if (left > 1u) test_sphere<COUNT>(r1, i1, ro, rd, a, inv_a, trace, closest, nb, work);
                            if (left > 2u) test_sphere<COUNT>(r2, i2, ro, rd, a, inv_a, trace, closest, nb, work);
                            if (left > 3u) test_sphere<COUNT>(r3, i3, ro, rd, a, inv_a, trace, closest, nb, work);
                        }
                    }
                    stamps.mark(3);
                } else {
                    grid_walk<COUNT, FLATY>(S, G, ro, rd, trace, resume, resume ? kWalkCellsResume : kWalkCellsFresh, closest, nb, walk_cell, cut, work, lane, stamps, GC);
                }
            } else {
                nb = nearest_hit<COUNT>(S, A.n_spheres, ro, rd, trace, closest, work);
                stamps.mark(5);                        // (diagnosis builds) the flat scan
            }
            const bool hit = trace && !cut && nb >= 0;
            if (hit) work.add(kCntHits);
            const uint32_t miss = (trace && !cut && nb < 0) ? 1u : 0u;        // left the scene: OP_GEN adds throughput x sky
#define MIRT_PROBE_SITE 5           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE
            // rayPointAtParameter (wgsl:442-444); unused after a miss; a cut walk keeps the ray's origin instead
            const f3 hp = cut ? ro : fma3(closest, rd, ro);
            // next routine, branch-free: the queue of a sphere's routine is kept with the sphere.  OP_GEN also when
            // the bounce limit ended the path.
            uint32_t hit_op;
            if constexpr (GRID) hit_op = 0u;              // the one scatter queue of a grid build
            else hit_op = S.spheres[hit ? nb : 0].op;
            const uint32_t new_op = alive ? (cut ? OP_WALK : (hit ? hit_op : OP_GEN)) : OP_NONE;

            // ---- fast-forward: all paths of this step wait for ONE routine -> run it on them now ----
            if constexpr (kFastForwardMin <= 64u) {
                const uint32_t k2 = __builtin_amdgcn_readfirstlane(new_op);      // lane 0 always holds a path (my_n >= 1)
                if (k2 != OP_NONE && my_n >= kFastForwardMin && ballot_(has && new_op != k2) == 0ull) {
                    ff = true;
                    my_k = k2;
                    ro = hp;
                    if constexpr (GRID) { best = (k2 == OP_WALK) ? nb : (nb < 0 ? 0 : nb); walk_closest = closest; }
                    else best = nb < 0 ? 0 : nb;
                    missf = miss;
                    continue;
                }
                ff = false;
            }

            if (has) {
                const uint32_t packed = (uint32_t)(nb < 0 ? 0 : nb) | (pix << 12) | (bounce << 16) | (miss << 24) | ((nb >= 0 ? 1u : 0u) << 25);
                L_state[slot * 3 + 0] = make_uint4(bits(hp.x), bits(hp.y), bits(hp.z), packed);
                L_state[slot * 3 + 1] = make_uint4(bits(rd.x), bits(rd.y), bits(rd.z), rng.state);
                if constexpr (PIXREC) *reinterpret_cast<uint3*>(&L_state[slot * 3 + 2]) = make_uint3(bits(thr.x), bits(thr.y), bits(thr.z));   // .w: a word of a pixel record
                else L_state[slot * 3 + 2] = make_uint4(bits(thr.x), bits(thr.y), bits(thr.z), GRID ? bits(closest) : 0u);
                if constexpr (GRID) { if (cut) L_cell[slot] = (unsigned short)walk_cell; }
            }
#define MIRT_PROBE_SITE 3           // experiment builds only: expands to nothing in libmirt.so
#include "mirt_pool_probes.inc"
#undef MIRT_PROBE_SITE
            // push every slot id to the queue of its next op (tails live in SGPRs: no atomics)
#pragma unroll
            for (uint32_t k = 0; k < kNumOps; ++k) {
                const unsigned long long mk_ = ballot_(new_op == k);
                // rank among the lanes of this queue = set bits of the ballot below this lane: v_mbcnt_lo + v_mbcnt_hi
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk_, 0u));
                if (new_op == k) L_ring[k * RING + tail[k] + rank] = (unsigned char)slot;
                tail[k] += (uint32_t)__popcll(mk_);
            }
        }

        // ---- strip finished: resolve and store 16 pixels with one coalesced 64-B write ----
        stamps.mark(9);
        stamps.flush(A.counters, lane);
        {
            const RenderArgs& AS = per_strip_args();
            if constexpr (FRAME) {               // progressive frame: add, and resolve the updated sums in the same pass.  Lane l owns ONE sum --
                // channel l % 3 of pixel l / 3 -- so it resolves that one channel (48 lanes busy with one channel each instead of 16
                // with three); the pixel's lane then collects its three codes from its neighbours.
                uint32_t code = 0u;
                if (lane < strip_pixels * 3) {
                    const unsigned long long sum = AS.accum[3ull * base_pix + lane] + L_acc[lane];
                    AS.accum[3ull * base_pix + lane] = sum;
                    code = resolve_channel(sum, AS.sample_begin + AS.spp, AS.flags);
                }
                const uint32_t src = (lane < kStripPixels ? lane : 0u) * 3u;
                const uint32_t r = (uint32_t)__shfl((int)code, (int)src, 64), g = (uint32_t)__shfl((int)code, (int)src + 1, 64),
                               b = (uint32_t)__shfl((int)code, (int)src + 2, 64);
                if (lane < strip_pixels) AS.out[base_pix + lane] = pack_rgba(r, g, b);
            } else if (AS.accum) {                      // progressive mode: add the exact sums, resolve later
                if (lane < strip_pixels * 3) AS.accum[3ull * base_pix + lane] += L_acc[lane];
            } else if (lane < strip_pixels) {
                const uint32_t rgba = pack_rgba(resolve_channel(L_acc[lane * 3 + 0], AS.spp, AS.flags),
                                                resolve_channel(L_acc[lane * 3 + 1], AS.spp, AS.flags),
                                                resolve_channel(L_acc[lane * 3 + 2], AS.spp, AS.flags));
                AS.out[base_pix + lane] = rgba;
            }
            work.flush(AS.counters, lane);
        }
    }
}
