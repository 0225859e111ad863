// mirt_pool_hbm_schedule.inc -- the pooled schedule of the BVH kernels, once: render_pt_pool_hbm_kernel / _frame_kernel
// (mirt_pool_hbm_kernel.inc, DESIGN.md 10.6), radiance_rays_pool_kernel (mirt_radiance_pool_kernel.inc, 10.11) and
// adapt_pixels_pool_kernel (mirt_adapt_pool_kernel.inc, 10.13).  Each of them includes the four parts below where the statements stand,
// selected by MIRT_POOL_HBM_PART -- shared TEXT, not shared functions: the same statements behind MIRT_DEV functions taking references
// changed the register allocation of every build (and cost 7.8 % in mirt_pool_kernel.inc, whose header has the figure); as text the
// kernels' code objects are byte for byte what they were with three copies (profiles/r21_isa_identity.md).
//
// The schedule is mirt_pool_kernel.inc's, specialised: a wave-private pool of SLOTS paths in LDS (WavePoolLayout<SLOTS, 1>), a unit of
// work items served by refilling finished slots, stack queues whose depths live in SGPRs, pick the deepest / pop / gather, the
// fast-forward of coherent steps, the ballot / mbcnt push, exact 64-bit sums in LDS.  What differs from that kernel:
//   * TWO queues, OP_GEN and ONE scatter queue (as in the grid build: the trace dominates a step).  The scatter step reads the sphere
//     and its material where they lie, in device memory, and shades with shade_by_id -- the per-lane switch, the arithmetic and the
//     draw order of path_radiance<SRC = kSrcBvh>.  No scene table is staged: LDS holds the camera (+ sky), the pools and the stacks.
//   * the common tail runs nearest_hit_bvh on the step's rays TO COMPLETION: no cut and resumed walks (parking a traversal needs a
//     stack per slot, not per lane), no candidate lists, no texel tiles.
//   * a sphere id needs 24 bits (MIRT_SCENE_HBM_MAX_SPHERES), which the state word's 12 do not hold: see PoolHbmState.
// mirt_pool_kernel.inc deliberately keeps its own copy: NQ queues, grid walks, tiles, pixel records, probes and stamps would need more
// hooks here than there are shared lines.
//
// An includer provides: COUNT, HOSEK, St = PoolHbmState, OP_SCATTER, OP_GEN, kNumOps, RING, SLOTS; A, S, lane, work, bvh_stack; L_state,
// L_acc, L_ring; and for part 4 MIRT_POOL_HBM_STATE_WORD, the fourth word of a slot's first vector (St::flags(pix, bounce, miss), or
// that with bits of the includer's own in the field PoolHbmState leaves free).  An includer whose paths carry more -- the adaptive
// kernel's second sums and their bit -- names both for part 1: MIRT_POOL_HBM_MORE_SUMS, a second [kStripPixels][3] array zeroed with
// L_acc, and MIRT_POOL_HBM_MORE_STATE, a loop-carried word declared behind missf.  They are hooks and not statements of the includer
// because an `if` or a declaration of its own behind part 1 moved instructions in its builds.  What is the includer's own: the unit
// loop, the unit's addressing, the OP_GEN routine (it sets alive, pix, ro, rd, rng, thr, bounce from next_item and adds the sky term
// of the path that ended) and the epilogue.
//   part 1  unit prologue, behind the includer's addressing : every slot into the OP_GEN queue, sums zeroed, the loop-carried state
//   part 2  the body of `if (!ff) { }`                      : pick the deepest queue (or leave the loop), pop, gather; fl = the state word
//   part 3  the body of the scatter step                    : sphere and material from device memory, shade_by_id
//   part 4  behind the two routines, to the loop's end      : bounce limit, nearest_hit_bvh, classification, fast-forward, store, push
#if MIRT_POOL_HBM_PART == 1
        // all slots start in the OP_GEN queue
        for (uint32_t s = lane; s < SLOTS; s += 64) { L_ring[OP_GEN * RING + s] = (unsigned char)s; L_state[s * 3].w = 0u; }
        if (lane < kStripPixels * 3) {
            L_acc[lane] = 0ull;
#ifdef MIRT_POOL_HBM_MORE_SUMS
            MIRT_POOL_HBM_MORE_SUMS[lane] = 0ull;
#endif
        }
        uint32_t tail[kNumOps];                            // queue depths, wave-uniform (SGPRs)
        tail[OP_SCATTER] = 0u;
        tail[OP_GEN] = SLOTS;
        uint32_t next_item = 0;

        // loop-carried path state of the lanes: loaded from the pool by a normal step, inherited by a fast-forward step
        bool ff = false;                                   // wave-uniform
        uint32_t my_k = 0, my_n = 0;                       // wave-uniform: routine of this step, number of paths
        uint32_t slot = 0, pix = 0, bounce = 0, missf = 0; // pix: the index in its unit of the path's pixel, ray or list entry
#ifdef MIRT_POOL_HBM_MORE_STATE
        uint32_t MIRT_POOL_HBM_MORE_STATE = 0;
#endif
        uint32_t best = 0;                                 // scatter steps: the sphere that was hit
        f3 ro = mk(0, 0, 0), rd = mk(0, 0, 0), thr = mk(0, 0, 0);
        Rng rng;
        rng.state = 0;
#elif MIRT_POOL_HBM_PART == 2
                // ---- pick the deepest queue: max over keys depth << 3 | (7 - op); ties go to the lower op ----
                const uint32_t key = deepest_key<0>(tail);
                const uint32_t depth = key >> 3;
                if (depth == 0) break;                     // every queue empty: unit finished
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
#elif MIRT_POOL_HBM_PART == 3
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
#elif MIRT_POOL_HBM_PART == 4
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
                L_state[slot * 3 + 0] = make_uint4(bits(hp.x), bits(hp.y), bits(hp.z), MIRT_POOL_HBM_STATE_WORD);
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
#else
#error "MIRT_POOL_HBM_PART: 1 (unit prologue), 2 (pick / pop / gather), 3 (scatter) or 4 (tail)"
#endif
