// mirt_radiance_pool_kernel.inc -- the pooled schedule for radiance queries (MIRT_RADIANCE_POOL on mirt_ctx_trace_radiance*; DESIGN.md
// 10.11).  Included once by mirt_kernels.hip behind mirt_radiance_kernel.inc, exact build only: no fast_build:: copy, no counting build.
//
// radiance_rays_pool_kernel<THREADS, SLOTS, MINW, HOSEK, SORTED> is the text of mirt_pool_hbm_kernel.inc -- a wave-private pool of SLOTS
// paths in LDS, two stack queues whose depths live in SGPRs, pick the deepest / pop / gather, the fast-forward of coherent steps, the
// ballot / mbcnt push, nearest_hit_bvh to completion on stacks as deep as the resident tree, shade_by_id on the sphere and material
// where they lie, exact 64-bit sums in LDS -- with three differences:
//   * a unit is kStripPixels = 16 consecutive SLOTS OF THE BATCH, not pixels: slot k is ray k, or ray order[k] when SORTED (the
//     permutation ray_sort_order left in device memory).  RenderArgs.n_units = ceil(n_rays / 16), RenderArgs.width = n_rays.  A unit's
//     work items are unit_rays x spp, item -> (sample = item / unit_rays, r = item % unit_rays); r takes the place of the pixel in
//     PoolHbmState::flags and in L_acc.  There are no strip levels and no camera.
//   * OP_GEN loads the item's ray from memory as radiance_rays_kernel does (two 16-byte loads: {origin, stream} {direction, _pad}), seeds
//     the stream of (stream, sample) and skips the four draws of a primary ray.  A lane without an item loads nothing.
//   * there is no dispenser: a wave takes unit first_unit(), then every grid_waves-th behind it.  The epilogue writes MirtRadiance
//     records (two 16-byte stores per ray, two loads in front of them under MIRT_RADIANCE_ACCUMULATE, as mirt_radiance_ray_body.inc):
//     no resolve, no counters.
// The sums are exact integers, so the order in which a unit's (ray, sample) items are served cannot change a byte: the records are those
// of radiance_rays_kernel.  LDS of a block is the pooled render's: camera words (+ sky) | THREADS / 64 pools | THREADS / 64 x 64 stacks
// of RenderArgs.bvh_stack_entries words -- mirt_bvh_pool_plan is the plan of this kernel too.
template <uint32_t THREADS, uint32_t SLOTS, uint32_t MINW, bool HOSEK, bool SORTED>
__global__ __launch_bounds__(THREADS, MINW) void radiance_rays_pool_kernel(RenderArgs A, const trace_u4* rays, trace_u4* out, const uint32_t* order)
{
    constexpr bool COUNT = false;
    using Lay = WavePoolLayout<SLOTS, 1>;
    using St = PoolHbmState;
    constexpr uint32_t OP_SCATTER = 0, OP_GEN = 1, kNumOps = Lay::kQueues;
    static_assert(kNumOps == 2, "OP_GEN and one scatter queue");
    constexpr uint32_t RING = Lay::kRing;
    static_assert(SLOTS >= 64 && SLOTS <= 256 && SLOTS % 8 == 0, "slot ids are 8 bit");
    static_assert(Lay::kBytes == bvh_pool_bytes_per_wave(SLOTS), "mirt_bvh_pool_plan's byte formula");
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, false>(A, smem, HOSEK);       // camera words (+ sky); S.spheres / S.pmats are the tables in device memory
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

    const uint32_t grid_waves = gridDim.x * (THREADS / 64u);
    for (uint32_t unit = first_unit(); unit < A.n_units; unit += grid_waves) {
        const RenderArgs& AP = per_strip_args();         // the arguments this prologue needs, loaded here and now
        const uint32_t base_slot = unit * kStripPixels;    // < n_rays: no overflow
        const uint32_t unit_rays = (AP.width - base_slot < kStripPixels) ? (AP.width - base_slot) : kStripPixels;
        const uint32_t total_items = unit_rays * AP.spp;

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
        uint32_t slot = 0, pix = 0, bounce = 0, missf = 0; // pix: the ray's index in its unit
        uint32_t best = 0;                                 // scatter steps: the sphere that was hit
        f3 ro = mk(0, 0, 0), rd = mk(0, 0, 0), thr = mk(0, 0, 0);
        Rng rng;
        rng.state = 0;

        for (;;) {
            if (!ff) {
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
            }
            const bool has = lane < my_n;
            bool alive = has;

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
                if (unit_rays == kStripPixels) { sample = item / kStripPixels; pix = item % kStripPixels; }
                else { sample = item / unit_rays; pix = item - sample * unit_rays; }      // ragged last unit
                // the item's ray, as radiance_rays_kernel loads it: {origin, stream} {direction, _pad}
                trace_u4 r0 = { 0u, 0u, 0u, 0u }, r1 = { 0u, 0u, 0u, 0u };
                if (alive) {
                    uint64_t i = base_slot + pix;
                    if constexpr (SORTED) i = order[i];
                    r0 = rays[2u * i];
                    r1 = rays[2u * i + 1u];
                }
                ro = mk(from_bits(r0.x), from_bits(r0.y), from_bits(r0.z));
                rd = mk(from_bits(r1.x), from_bits(r1.y), from_bits(r1.z));
                // generate_primary's seed with `stream` for the pixel index, then the two jitter and the two lens draws of a primary ray
                rng.state = jenkins_hash((r0.w ^ jenkins_hash(A.sample_begin + sample + 1u)) ^ A.seed_mix);
                rng.skip(); rng.skip(); rng.skip(); rng.skip();
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

        // ---- unit finished: lane r < unit_rays owns the record of the unit's r-th slot ----
        if (lane < unit_rays) {
            const RenderArgs& AS = per_strip_args();
            uint64_t i = base_slot + lane;
            if constexpr (SORTED) i = order[i];
            unsigned long long acc_r = L_acc[lane * 3 + 0], acc_g = L_acc[lane * 3 + 1], acc_b = L_acc[lane * 3 + 2];
            uint32_t samples = AS.spp;
            if (AS.flags & kRadianceAccumulate) {
                const trace_u4 o0 = out[2u * i], o1 = out[2u * i + 1u];
                acc_r += (unsigned long long)o0.x | ((unsigned long long)o0.y << 32);
                acc_g += (unsigned long long)o0.z | ((unsigned long long)o0.w << 32);
                acc_b += (unsigned long long)o1.x | ((unsigned long long)o1.y << 32);
                samples += o1.z;
            }
            out[2u * i] = trace_u4{ (uint32_t)acc_r, (uint32_t)(acc_r >> 32), (uint32_t)acc_g, (uint32_t)(acc_g >> 32) };
            out[2u * i + 1u] = trace_u4{ (uint32_t)acc_b, (uint32_t)(acc_b >> 32), samples, 0u };
        }
    }
}

// ---- one build per geometry of kBvhPoolSlotChoices (the pooled HBM render's table) x HOSEK x SORTED ----
using RadiancePoolKernel = void (*)(RenderArgs, const trace_u4*, trace_u4*, const uint32_t*);
template <uint32_t SL>
static RadiancePoolKernel radiance_pool_kernel_(bool hosek, bool sorted)
{
    constexpr uint32_t T = kBvhPoolThreads, MW = kBvhPoolMinWaves;
    return hosek ? (sorted ? radiance_rays_pool_kernel<T, SL, MW, true, true> : radiance_rays_pool_kernel<T, SL, MW, true, false>)
                 : (sorted ? radiance_rays_pool_kernel<T, SL, MW, false, true> : radiance_rays_pool_kernel<T, SL, MW, false, false>);
}

static RadiancePoolKernel radiance_pool_kernel(uint32_t slots, bool hosek, bool sorted)
{
    if (slots == kBvhPoolSlotChoices[0]) return radiance_pool_kernel_<kBvhPoolSlotChoices[0]>(hosek, sorted);
    if (slots == kBvhPoolSlotChoices[1]) return radiance_pool_kernel_<kBvhPoolSlotChoices[1]>(hosek, sorted);
    if (slots == kBvhPoolSlotChoices[2]) return radiance_pool_kernel_<kBvhPoolSlotChoices[2]>(hosek, sorted);
    if (slots == kBvhPoolSlotChoices[3]) return radiance_pool_kernel_<kBvhPoolSlotChoices[3]>(hosek, sorted);
    return nullptr;
}

// a.n_units units of 16 slots (a.width rays), grid_blocks blocks of kBvhPoolThreads; a.lds_bytes = mirt_bvh_pool_plan's bytes per block,
// a.bvh_stack_entries its stack entries; d_order: the permutation (MIRT_RADIANCE_SORT) or nullptr
hipError_t launch_radiance_pool(const RenderArgs& a, const void* d_rays, void* d_out, const uint32_t* d_order, uint32_t grid_blocks, uint32_t slots, bool hosek,
                                hipStream_t stream)
{
    const RadiancePoolKernel k = radiance_pool_kernel(slots, hosek, d_order != nullptr);
    if (!k) return hipErrorInvalidValue;
    if (a.lds_bytes > 48u * 1024u) {        // more than the default dynamic-LDS window: ask for it (launch_with_lds)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(grid_blocks), dim3(kBvhPoolThreads), a.lds_bytes, stream, a, static_cast<const trace_u4*>(d_rays), static_cast<trace_u4*>(d_out), d_order);
    return hipGetLastError();
}
