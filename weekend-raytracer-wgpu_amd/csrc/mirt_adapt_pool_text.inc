// mirt_adapt_pool_text.inc -- the pooled render stage of an adaptive step, as TEXT: mirt_adapt_pool_kernel.inc, whose header describes the
// kernel, includes it twice.
//   MIRT_ADAPT_POOL_KERNEL   the kernel's name: adapt_pixels_pool_kernel (a step) or adapt_pixels_pool_run_kernel (a step of a run)
//   MIRT_ADAPT_RUN           0: a list entry's sample count is the launch's (AP.spp / AS.spp, re-read from the kernel arguments per unit)
//                            1: it is the word behind the count (head[1], which adapt_scan_run_kernel wrote for this step), read once as
//                               a wave-uniform word next to the count, before anything is staged (DESIGN.md 10.14)
// Text and not a template parameter, as the schedule itself is: adapt_pixels_pool_kernel<THREADS, SLOTS, MINW, HOSEK> keeps its name and,
// token for token, its code.
template <uint32_t THREADS, uint32_t SLOTS, uint32_t MINW, bool HOSEK>
__global__ __launch_bounds__(THREADS, MINW) void MIRT_ADAPT_POOL_KERNEL(RenderArgs A, adapt_u4* recs, const uint32_t* list, const uint32_t* count_word)
{
    constexpr bool COUNT = false;
    using Lay = WavePoolLayout<SLOTS, 1>;
    using St = PoolHbmState;
    using Sa = AdaptPoolState;
    constexpr uint32_t OP_SCATTER = 0, OP_GEN = 1, kNumOps = Lay::kQueues;
    static_assert(kNumOps == 2, "OP_GEN and one scatter queue");
    constexpr uint32_t RING = Lay::kRing;
    static_assert(SLOTS >= 64 && SLOTS <= 256 && SLOTS % 8 == 0, "slot ids are 8 bit");
    // a wave's LDS: the schedule's pool | even [kStripPixels][3] u64 | table [kStripPixels] {place, samples}
    constexpr uint32_t kOffEven = Lay::kBytes, kOffTable = kOffEven + kStripPixels * 3u * 8u, kWaveBytes = kOffTable + kStripPixels * 8u;
    static_assert(kOffEven % 16u == 0u, "the even sums and the table are 8-byte words behind a 16-byte aligned pool");
    static_assert(kWaveBytes == Lay::kBytes + kAdaptPoolExtraBytes && kWaveBytes == adapt_pool_bytes_per_wave(SLOTS), "mirt_adapt_pool_plan's byte formula");

    const uint32_t count = __builtin_amdgcn_readfirstlane(*count_word);
#if MIRT_ADAPT_RUN
    // a unit holds up to 16 x step_spp <= 16 << 24 items: next_item, total_items and item are 32 bit, and next_item overshoots
    // total_items by less than SLOTS
    static_assert(((uint64_t)kStripPixels << 24) + 256u < (1ull << 32) && MIRT_MAX_SPP_PER_CALL == (1u << 24), "a unit's item counters are 32 bit");
    const uint32_t step_spp = __builtin_amdgcn_readfirstlane(count_word[1]);      // 0 exactly when count is 0
#define MIRT_ADAPT_SPP(ARGS) ((void)(ARGS), step_spp)
#else
#define MIRT_ADAPT_SPP(ARGS) (ARGS).spp
#endif
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
        const uint32_t total_items = unit_entries * MIRT_ADAPT_SPP(AP);

        // the unit's table: entry r -> {its record's place in the band, the samples it holds}; entries beyond a ragged unit read as {0, 0}
        if (lane < kStripPixels) {
            uint2 e = make_uint2(0u, 0u);
            if (lane < unit_entries) {
                e.x = list[base_entry + lane];             // < out_rows x width (adapt_compact_kernel)
                e.y = recs[4ull * e.x + 3u].x;
            }
            L_table[lane] = e;
        }
#define MIRT_POOL_HBM_MORE_SUMS L_even  // zeroed with L_acc
#define MIRT_POOL_HBM_MORE_STATE evenf  // loop-carried with missf: was the path's sample index even?
#define MIRT_POOL_HBM_PART 1           // every slot into the OP_GEN queue, sums zeroed; tail[], next_item and the loop-carried state
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
#undef MIRT_POOL_HBM_MORE_STATE
#undef MIRT_POOL_HBM_MORE_SUMS

        for (;;) {
            if (!ff) {
#define MIRT_POOL_HBM_PART 2           // pick the deepest queue (or leave the loop), pop, gather; fl = the state word
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
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
#define MIRT_POOL_HBM_PART 3           // sphere and material from device memory, shade_by_id
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
            }

#define MIRT_POOL_HBM_STATE_WORD Sa::flags(pix, bounce, miss, evenf)
#define MIRT_POOL_HBM_PART 4           // bounce limit, nearest_hit_bvh, classification, fast-forward, store, push
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
#undef MIRT_POOL_HBM_STATE_WORD
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
            recs[4u * pi + 3u] = adapt_u4{ e.y + MIRT_ADAPT_SPP(AS), 0u, 0u, 0u };
        }
    }
}
#undef MIRT_ADAPT_SPP
