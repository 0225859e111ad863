// mirt_pool_hbm_kernel.inc -- the text of the pooled path-traced kernel of MIRT_SCENE_HBM scenes (MIRT_FLAG_KERNEL_POOL on such a
// scene; DESIGN.md 10.6).  mirt_kernels.hip includes it twice:
//   MIRT_POOL_HBM_KERNEL_NAME = render_pt_pool_hbm_kernel,       MIRT_POOL_HBM_KERNEL_FRAME = false
//   MIRT_POOL_HBM_KERNEL_NAME = render_pt_pool_hbm_frame_kernel, MIRT_POOL_HBM_KERNEL_FRAME = true   (the progressive-frame build)
// The schedule is mirt_pool_kernel.inc's: a wave-private pool of SLOTS paths in LDS, 16-pixel strips x spp as work items, the guided
// strip levels and the dispenser, stack queues whose depths live in SGPRs, pick the deepest / pop / gather, the fast-forward of
// coherent steps, the ballot / mbcnt push and the three epilogues.  What differs:
//   * TWO queues, OP_GEN and ONE scatter queue (as in the grid build: the trace dominates a step).  The scatter step reads the sphere
//     and its material where they lie, in device memory, and shades with shade_by_id -- the per-lane switch, the arithmetic and the
//     draw order of path_radiance<SRC = kSrcBvh>.  No scene table is staged: LDS holds the camera (+ sky), the pools and the stacks.
//   * the common tail runs nearest_hit_bvh on the step's rays TO COMPLETION: no cut and resumed walks (parking a traversal needs a
//     stack per slot, not per lane), no candidate lists, no texel tiles.
//   * a sphere id needs 24 bits (MIRT_SCENE_HBM_MAX_SPHERES), which the state word's 12 do not hold: see PoolHbmState.
//   * behind the block's pools every wave has 64 traversal stacks of RenderArgs.bvh_stack_entries node references -- the depth of the
//     RESIDENT tree, not MIRT_BVH_MAX_DEPTH: 256 x depth bytes per wave (mirt_bvh_pool_plan).
template <uint32_t THREADS, uint32_t SLOTS, uint32_t MINW, bool COUNT, bool HOSEK>
__global__ __launch_bounds__(THREADS, MINW) void MIRT_POOL_HBM_KERNEL_NAME(RenderArgs A)
{
    constexpr bool FRAME = MIRT_POOL_HBM_KERNEL_FRAME;
    using Lay = WavePoolLayout<SLOTS, 1>;
    using St = PoolHbmState;
    constexpr uint32_t OP_SCATTER = 0, OP_GEN = 1, kNumOps = Lay::kQueues;
    static_assert(kNumOps == 2, "OP_GEN and one scatter queue");
    constexpr uint32_t RING = Lay::kRing;
    static_assert(SLOTS >= 64 && SLOTS <= 256 && SLOTS % 8 == 0, "slot ids are 8 bit");
    static_assert(Lay::kBytes == bvh_pool_bytes_per_wave(SLOTS), "mirt_bvh_pool_plan's byte formula");
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, false>(A, smem, HOSEK);       // camera (+ sky); S.spheres / S.pmats are the tables in device memory
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t scene_bytes = (uint32_t)scene_lds_bytes_dev(0u, 0u, HOSEK, false);
    // LDS of a block: camera (+ sky) | [THREADS / 64] pools | [THREADS / 64] x 64 traversal stacks of bvh_stack_entries words, lane-interleaved
    unsigned char* pool = smem + scene_bytes + wave * Lay::kBytes;
    uint32_t* const bvh_stack = reinterpret_cast<uint32_t*>(smem + scene_bytes + (THREADS / 64u) * Lay::kBytes) + wave * (64u * A.bvh_stack_entries);
    uint4* const L_state = reinterpret_cast<uint4*>(pool + Lay::kOffState);
    unsigned long long* const L_acc = reinterpret_cast<unsigned long long*>(pool + Lay::kOffAcc);
    unsigned char* const L_ring = pool + Lay::kOffRing;

    Work<COUNT> work;
    work.clear();

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
        uint32_t tail[kNumOps];                            // queue depths, wave-uniform (SGPRs)
        tail[OP_SCATTER] = 0u;
        tail[OP_GEN] = SLOTS;
        uint32_t next_item = 0;

        // loop-carried path state of the lanes: loaded from the pool by a normal step, inherited by a fast-forward step
        bool ff = false;                                   // wave-uniform
        uint32_t my_k = 0, my_n = 0;                       // wave-uniform: routine of this step, number of paths
        uint32_t slot = 0, pix = 0, bounce = 0, missf = 0;
        uint32_t best = 0;                                 // scatter steps: the sphere that was hit
        f3 ro = mk(0, 0, 0), rd = mk(0, 0, 0), thr = mk(0, 0, 0);
        Rng rng;
        rng.state = 0;

        for (;;) {
            if (!ff) {
                // ---- pick the deepest queue: max over keys depth << 3 | (7 - op); ties go to the lower op ----
                const uint32_t key = deepest_key<0>(tail);
                const uint32_t depth = key >> 3;
                if (depth == 0) break;                     // every queue empty: strip finished
                my_k = 7u - (key & 7u);
                my_n = (depth > 64u) ? 64u : depth;
                const uint32_t my_begin = depth - my_n;    // the top my_n entries
#pragma unroll
                for (uint32_t k = 0; k < kNumOps; ++k) tail[k] -= (my_k == k) ? my_n : 0u;

                // ---- pop + gather ----
                const bool has0 = lane < my_n;
                slot = has0 ? (uint32_t)L_ring[my_k * RING + my_begin + lane] : 0u;
                const uint4 q0 = L_state[slot * 3 + 0], q1 = L_state[slot * 3 + 1], q2 = L_state[slot * 3 + 2];
                const uint32_t fl = q0.w;
                ro = mk(from_bits(q0.x), from_bits(q0.y), from_bits(q0.z));      // the hit point for scatter steps
                rd = mk(from_bits(q1.x), from_bits(q1.y), from_bits(q1.z));
                thr = mk(from_bits(q2.x), from_bits(q2.y), from_bits(q2.z));
                best = has0 ? St::id(q2.w) : 0u;
                rng.state = q1.w;
                pix = St::pixel(fl);
                bounce = St::bounce(fl);
                missf = St::miss(fl);
            }
            const bool has = lane < my_n;
            bool alive = has;
            if constexpr (COUNT) { if (lane == 0) work.add(kCntWaveIters); }

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
                // pixel -> (x, y): the strip starts at (base_x, row0) and may wrap into following rows
                uint32_t x = base_x + pix, y = row0;
                if (wide) { if (x >= A.width) { x -= A.width; y = row1; } }
                else { const uint32_t pi = base_pix + pix; const uint32_t ci = pi / A.width; x = pi - ci * A.width; y = abs_row(A, ci); }
                const CamRegs C = load_camera(S, A);       // re-read from LDS per GEN step instead of living in VGPRs across the kernel
                generate_primary(A, C, x, y, A.sample_begin + sample, rng, ro, rd);
                thr = mk(1, 1, 1);
                bounce = 0;
            } else {
                // sphereIntersection wgsl:431-440, then scatterRay's switch per lane: path_radiance's statements for SRC == kSrcBvh, on the
                // lanes that hold a path (an idle lane reads nothing from device memory)
                const f3 hp = ro;                          // computed by the tail of the step that found the hit
                f3 ndir = rd, att = mk(1, 1, 1);
                if (has) {
                    const PreparedSphere sp = S.spheres[best];
                    const f3 hn = sp.inv_r * (hp - mk(sp.cx, sp.cy, sp.cz));
                    const PreparedMaterial* m = &S.pmats[sp.material_idx];
                    const Scattered sc = shade_by_id<COUNT>(A, m, m->id, true, rd, hp, hn, rng, work);
                    ndir = sc.dir;
                    att = sc.att;
                }
                rd = ndir;
                thr = thr * att;
                bounce += 1;
            }

            // common tail: bounce limit (wgsl:130), nearest hit through the tree, classification
            const bool trace = alive && bounce < A.num_bounces;
            if constexpr (COUNT) { if (trace) work.add(kCntLaneIters); }
            float closest;
            const int nb = nearest_hit_bvh<COUNT>(ro, rd, trace, closest, work, lane, bvh_stack, A.bvh_stack_entries);
            const bool hit = trace && nb >= 0;
            if (hit) work.add(kCntHits);
            const uint32_t miss = (trace && nb < 0) ? 1u : 0u;        // left the scene: OP_GEN adds throughput x sky
            const f3 hp = fma3(closest, rd, ro);           // rayPointAtParameter (wgsl:442-444); unused after a miss
            // OP_GEN also when the bounce limit ended the path
            const uint32_t new_op = alive ? (hit ? OP_SCATTER : OP_GEN) : OP_NONE;

            // ---- fast-forward: all paths of this step wait for ONE routine -> run it on them now ----
            if constexpr (kFastForwardMin <= 64u) {
                const uint32_t k2 = __builtin_amdgcn_readfirstlane(new_op);      // lane 0 always holds a path (my_n >= 1)
                if (k2 != OP_NONE && my_n >= kFastForwardMin && ballot_(has && new_op != k2) == 0ull) {
                    ff = true;
                    my_k = k2;
                    ro = hp;
                    best = nb < 0 ? 0u : (uint32_t)nb;
                    missf = miss;
                    continue;
                }
                ff = false;
            }

            if (has) {
                L_state[slot * 3 + 0] = make_uint4(bits(hp.x), bits(hp.y), bits(hp.z), St::flags(pix, bounce, miss));
                L_state[slot * 3 + 1] = make_uint4(bits(rd.x), bits(rd.y), bits(rd.z), rng.state);
                L_state[slot * 3 + 2] = make_uint4(bits(thr.x), bits(thr.y), bits(thr.z), St::hit_word(nb));
            }
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
        {
            const RenderArgs& AS = per_strip_args();
            if constexpr (FRAME) {               // progressive frame: add, and resolve the updated sums in the same pass (mirt_pool_kernel.inc)
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
