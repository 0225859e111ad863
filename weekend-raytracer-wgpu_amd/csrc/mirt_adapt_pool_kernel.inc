// mirt_adapt_pool_kernel.inc -- the pooled schedule for adaptive steps (MIRT_ADAPT_POOL on mirt_ctx_adapt_step_device; DESIGN.md 10.13).
// Included once by mirt_kernels.hip behind mirt_adapt_kernel.inc, exact build only: no fast_build:: copy, no counting build.
//
// adapt_pixels_pool_kernel<THREADS, SLOTS, MINW, HOSEK> is the text of radiance_rays_pool_kernel (mirt_radiance_pool_kernel.inc) -- a
// wave-private pool of SLOTS paths in LDS, two stack queues whose depths live in SGPRs, pick the deepest / pop / gather, the
// fast-forward of coherent steps, the ballot / mbcnt push, nearest_hit_bvh to completion on stacks as deep as the resident tree,
// shade_by_id on the sphere and material where they lie, exact 64-bit sums in LDS -- with these differences:
//   * a unit is kStripPixels = 16 consecutive entries of the step's LIST.  The count is known on the device only: it is read as a
//     wave-uniform word, n_units = ceil(count / 16), and a block whose first unit lies beyond returns before anything is staged and
//     before any barrier, the whole block.  A unit's work items are unit_entries x spp, item -> (s = item / unit_entries,
//     r = item % unit_entries); r takes the place of the pixel in PoolHbmState::flags and in the accumulators.
//   * behind the pool of WavePoolLayout<SLOTS, 1> a wave keeps kAdaptPoolExtraBytes more: the 16 x 3 `even` accumulators and a table
//     {place in the band, samples so far} of its 16 entries, which the unit's prologue fills from the list and the records.
//   * OP_GEN derives the item's pixel from the table -- x, y = abs_row(place / width) -- and calls generate_primary with the camera
//     re-read from LDS for sample n + s of that pixel's stream, as adapt_pixels_kernel does.  A path carries one bit more than the
//     parent's: whether its sample index n + s is even (AdaptPoolState, bit 25 of the state word, free in PoolHbmState); its sky term is
//     added to `sum` and, with the bit set, to `even`.
//   * there is no dispenser: a wave takes unit first_unit(), then every grid_waves-th behind it.  The epilogue loads the sums of entry
//     r's record (three 16-byte loads; its count n is the table's, read by the prologue from the fourth quarter), adds the six sums, sets
//     samples = n + spp, writes the pads as 0 and stores four 16-byte quarters.
// The sums are exact integers, so the order in which a unit's (entry, sample) items are served cannot change a byte: the records are
// those of adapt_pixels_kernel.  LDS of a block: camera words (+ sky) | THREADS / 64 pools of adapt_pool_bytes_per_wave(SLOTS) |
// THREADS / 64 x 64 stacks of RenderArgs.bvh_stack_entries words -- mirt_adapt_pool_plan is the plan of this kernel.

// PoolHbmState's state word with the parity of the path's sample index in a bit that struct leaves free (25 .. 30)
struct AdaptPoolState {
    static constexpr uint32_t kEvenShift = 25;
    static_assert(kEvenShift > PoolHbmState::kMissShift && kEvenShift < PoolHbmState::kHitShift, "a bit PoolHbmState::flags never sets");
    static MIRT_DEV uint32_t flags(uint32_t r, uint32_t bounce, uint32_t miss, uint32_t even) { return PoolHbmState::flags(r, bounce, miss) | (even << kEvenShift); }
    static MIRT_DEV uint32_t even(uint32_t fl) { return (fl >> kEvenShift) & 1u; }
};

template <uint32_t THREADS, uint32_t SLOTS, uint32_t MINW, bool HOSEK>
__global__ __launch_bounds__(THREADS, MINW) void adapt_pixels_pool_kernel(RenderArgs A, adapt_u4* recs, const uint32_t* list, const uint32_t* count_word)
{
    constexpr bool COUNT = false;
    using Lay = WavePoolLayout<SLOTS, 1>;
    using St = PoolHbmState;
    using Sa = AdaptPoolState;
    constexpr uint32_t OP_SCATTER = 0, OP_GEN = 1, kNumOps = Lay::kQueues;
    static_assert(kNumOps == 2, "OP_GEN and one scatter queue");
    constexpr uint32_t RING = Lay::kRing;
    static_assert(SLOTS >= 64 && SLOTS <= 256 && SLOTS % 8 == 0, "slot ids are 8 bit");
    // a wave's LDS: the parent's pool | even [kStripPixels][3] u64 | table [kStripPixels] {place, samples}
    constexpr uint32_t kOffEven = Lay::kBytes, kOffTable = kOffEven + kStripPixels * 3u * 8u, kWaveBytes = kOffTable + kStripPixels * 8u;
    static_assert(kOffEven % 16u == 0u, "the even sums and the table are 8-byte words behind a 16-byte aligned pool");
    static_assert(kWaveBytes == Lay::kBytes + kAdaptPoolExtraBytes && kWaveBytes == adapt_pool_bytes_per_wave(SLOTS), "mirt_adapt_pool_plan's byte formula");

    const uint32_t count = __builtin_amdgcn_readfirstlane(*count_word);
    const uint32_t n_units = (count >> 4) + ((count & (kStripPixels - 1u)) != 0u ? 1u : 0u);        // ceil(count / 16) without overflow
    static_assert(kStripPixels == 16u, "a unit is 16 list entries");
    if (blockIdx.x * (THREADS / 64u) >= n_units) return;              // the whole block: nothing staged, no barrier met
    extern __shared__ __align__(16) unsigned char smem[];
    const SceneLds S = stage_scene<true, false>(A, smem, HOSEK);       // camera words (+ sky); S.spheres / S.pmats are the tables in device memory
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t scene_bytes = (uint32_t)scene_lds_bytes_dev(0u, 0u, HOSEK, false);
    // LDS of a block: camera (+ sky) | [THREADS / 64] pools | [THREADS / 64] x 64 traversal stacks of bvh_stack_entries words, lane-interleaved
    unsigned char* pool = smem + scene_bytes + wave * kWaveBytes;
    uint32_t* const bvh_stack = reinterpret_cast<uint32_t*>(smem + scene_bytes + (THREADS / 64u) * kWaveBytes) + wave * (64u * A.bvh_stack_entries);
    uint4* const L_state = reinterpret_cast<uint4*>(pool + Lay::kOffState);
    unsigned long long* const L_acc = reinterpret_cast<unsigned long long*>(pool + Lay::kOffAcc);
    unsigned char* const L_ring = pool + Lay::kOffRing;
    unsigned long long* const L_even = reinterpret_cast<unsigned long long*>(pool + kOffEven);
    uint2* const L_table = reinterpret_cast<uint2*>(pool + kOffTable);

    Work<COUNT> work;
    work.clear();

    const uint32_t grid_waves = gridDim.x * (THREADS / 64u);
    for (uint32_t unit = first_unit(); unit < n_units; unit += grid_waves) {
        const RenderArgs& AP = per_strip_args();         // the arguments this prologue needs, loaded here and now
        const uint32_t base_entry = unit * kStripPixels;   // < count: no overflow
        const uint32_t unit_entries = (count - base_entry < kStripPixels) ? (count - base_entry) : kStripPixels;
        const uint32_t total_items = unit_entries * AP.spp;

        // the unit's table: entry r -> {its record's place in the band, the samples it holds}; entries beyond a ragged unit read as {0, 0}
        if (lane < kStripPixels) {
            uint2 e = make_uint2(0u, 0u);
            if (lane < unit_entries) {
                e.x = list[base_entry + lane];             // < out_rows x width (adapt_compact_kernel)
                e.y = recs[4ull * e.x + 3u].x;
            }
            L_table[lane] = e;
        }
        // all slots start in the OP_GEN queue
        for (uint32_t s = lane; s < SLOTS; s += 64) { L_ring[OP_GEN * RING + s] = (unsigned char)s; L_state[s * 3].w = 0u; }
        if (lane < kStripPixels * 3) { L_acc[lane] = 0ull; L_even[lane] = 0ull; }
        uint32_t tail[kNumOps];                            // queue depths, wave-uniform (SGPRs)
        tail[OP_SCATTER] = 0u;
        tail[OP_GEN] = SLOTS;
        uint32_t next_item = 0;

        // loop-carried path state of the lanes: loaded from the pool by a normal step, inherited by a fast-forward step
        bool ff = false;                                   // wave-uniform
        uint32_t my_k = 0, my_n = 0;                       // wave-uniform: routine of this step, number of paths
        uint32_t slot = 0, pix = 0, bounce = 0, missf = 0, evenf = 0;      // pix: the entry's index in its unit
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
                evenf = Sa::even(fl);
            }
            const bool has = lane < my_n;
            bool alive = has;

            if (my_k == OP_GEN) {
                // finish the previous path of this slot: its sky term goes to `sum`, and to `even` when its sample index was even ...
                if (has && missf) {
                    work.add(kCntSky);
                    const f3 c = sky_color<HOSEK>(S, rd);
                    const unsigned long long fr = to_fixed(thr.x * c.x), fg = to_fixed(thr.y * c.y), fb = to_fixed(thr.z * c.z);
                    atomicAdd(&L_acc[pix * 3 + 0], fr);
                    atomicAdd(&L_acc[pix * 3 + 1], fg);
                    atomicAdd(&L_acc[pix * 3 + 2], fb);
                    if (evenf) {
                        atomicAdd(&L_even[pix * 3 + 0], fr);
                        atomicAdd(&L_even[pix * 3 + 1], fg);
                        atomicAdd(&L_even[pix * 3 + 2], fb);
                    }
                }
                // ... and start the next work item in it
                const uint32_t item = next_item + lane;
                next_item += my_n;
                alive = has && item < total_items;
                uint32_t sample;
                if (unit_entries == kStripPixels) { sample = item / kStripPixels; pix = item % kStripPixels; }
                else { sample = item / unit_entries; pix = item - sample * unit_entries; }      // ragged last unit
                // the item's pixel and the samples it holds, from the unit's table (pix < 16 on every lane)
                const uint2 e = L_table[pix];
                const uint32_t ci = e.x / A.width;
                const uint32_t x = e.x - ci * A.width;
                const uint32_t y = abs_row(A, ci);
                const uint32_t index = e.y + sample;       // sample n + s of the pixel's own stream
                {   // camera constants are re-read from LDS per GEN step instead of living in VGPRs across the kernel
                    const CamRegs C = load_camera(S, A);
                    generate_primary(A, C, x, y, index, rng, ro, rd);
                }
                thr = mk(1, 1, 1);
                bounce = 0;
                evenf = (index & 1u) ^ 1u;
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
                L_state[slot * 3 + 0] = make_uint4(bits(hp.x), bits(hp.y), bits(hp.z), Sa::flags(pix, bounce, miss, evenf));
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

        // ---- unit finished: lane r < unit_entries owns the record of the unit's r-th entry ----
        if (lane < unit_entries) {
            const RenderArgs& AS = per_strip_args();
            const uint2 e = L_table[lane];
            const uint64_t pi = e.x;
            const adapt_u4 q0 = recs[4u * pi], q1 = recs[4u * pi + 1u], q2 = recs[4u * pi + 2u];
            const unsigned long long sum_r = adapt_u64(q0.x, q0.y) + L_acc[lane * 3 + 0], sum_g = adapt_u64(q0.z, q0.w) + L_acc[lane * 3 + 1],
                                     sum_b = adapt_u64(q1.x, q1.y) + L_acc[lane * 3 + 2];
            const unsigned long long even_r = adapt_u64(q1.z, q1.w) + L_even[lane * 3 + 0], even_g = adapt_u64(q2.x, q2.y) + L_even[lane * 3 + 1],
                                     even_b = adapt_u64(q2.z, q2.w) + L_even[lane * 3 + 2];
            recs[4u * pi] = adapt_u4{ (uint32_t)sum_r, (uint32_t)(sum_r >> 32), (uint32_t)sum_g, (uint32_t)(sum_g >> 32) };
            recs[4u * pi + 1u] = adapt_u4{ (uint32_t)sum_b, (uint32_t)(sum_b >> 32), (uint32_t)even_r, (uint32_t)(even_r >> 32) };
            recs[4u * pi + 2u] = adapt_u4{ (uint32_t)even_g, (uint32_t)(even_g >> 32), (uint32_t)even_b, (uint32_t)(even_b >> 32) };
            recs[4u * pi + 3u] = adapt_u4{ e.y + AS.spp, 0u, 0u, 0u };
        }
    }
}

// ---- one build per geometry of kBvhPoolSlotChoices (the pooled HBM render's table) x HOSEK ----
using AdaptPoolKernel = void (*)(RenderArgs, adapt_u4*, const uint32_t*, const uint32_t*);
template <uint32_t SL>
static AdaptPoolKernel adapt_pool_kernel_(bool hosek)
{
    constexpr uint32_t T = kBvhPoolThreads, MW = kBvhPoolMinWaves;
    return hosek ? adapt_pixels_pool_kernel<T, SL, MW, true> : adapt_pixels_pool_kernel<T, SL, MW, false>;
}

static AdaptPoolKernel adapt_pool_kernel(uint32_t slots, bool hosek)
{
    if (slots == kBvhPoolSlotChoices[0]) return adapt_pool_kernel_<kBvhPoolSlotChoices[0]>(hosek);
    if (slots == kBvhPoolSlotChoices[1]) return adapt_pool_kernel_<kBvhPoolSlotChoices[1]>(hosek);
    if (slots == kBvhPoolSlotChoices[2]) return adapt_pool_kernel_<kBvhPoolSlotChoices[2]>(hosek);
    if (slots == kBvhPoolSlotChoices[3]) return adapt_pool_kernel_<kBvhPoolSlotChoices[3]>(hosek);
    return nullptr;
}

// The render stage of a pooled step: grid_blocks blocks of kBvhPoolThreads, whose waves stride over the units of 16 list entries; a.lds_bytes =
// mirt_adapt_pool_plan's bytes per block, a.bvh_stack_entries its stack entries
hipError_t launch_adapt_pixels_pool(const RenderArgs& a, void* d_recs, const uint32_t* d_list, const uint32_t* d_count, uint32_t grid_blocks, uint32_t slots, bool hosek,
                                    hipStream_t stream)
{
    const AdaptPoolKernel k = adapt_pool_kernel(slots, hosek);
    if (!k) return hipErrorInvalidValue;
    if (a.lds_bytes > 48u * 1024u) {        // more than the default dynamic-LDS window: ask for it (launch_radiance_pool)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(grid_blocks), dim3(kBvhPoolThreads), a.lds_bytes, stream, a, static_cast<adapt_u4*>(d_recs), d_list, d_count);
    return hipGetLastError();
}
