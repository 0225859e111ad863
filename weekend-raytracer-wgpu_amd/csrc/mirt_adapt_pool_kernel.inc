// mirt_adapt_pool_kernel.inc -- the pooled schedule for adaptive steps (MIRT_ADAPT_POOL on mirt_ctx_adapt_step_device; DESIGN.md 10.13).
// Included once by mirt_kernels.hip behind mirt_adapt_kernel.inc, exact build only: no fast_build:: copy, no counting build.
//
// The schedule of adapt_pixels_pool_kernel<THREADS, SLOTS, MINW, HOSEK> is mirt_pool_hbm_schedule.inc; this file holds what is the
// kernel's own:
//   * a unit is kStripPixels = 16 consecutive entries of the step's LIST.  The count is known on the device only: it is read as a
//     wave-uniform word, n_units = ceil(count / 16), and a block whose first unit lies beyond returns before anything is staged and
//     before any barrier, the whole block.  A unit's work items are unit_entries x spp, item -> (s = item / unit_entries,
//     r = item % unit_entries); r takes the place of the pixel in PoolHbmState::flags and in the accumulators.
//   * behind the pool of WavePoolLayout<SLOTS, 1> a wave keeps kAdaptPoolExtraBytes more: the 16 x 3 `even` accumulators and a table
//     {place in the band, samples so far} of its 16 entries, which the unit's prologue fills from the list and the records.
//   * OP_GEN derives the item's pixel from the table -- x, y = abs_row(place / width) -- and calls generate_primary with the camera
//     re-read from LDS for sample n + s of that pixel's stream, as adapt_pixels_kernel does.  A path carries one bit more than the
//     schedule's: whether its sample index n + s is even (AdaptPoolState, bit 25 of the state word, free in PoolHbmState); its sky term
//     is added to `sum` and, with the bit set, to `even`.
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
    // a wave's LDS: the schedule's pool | even [kStripPixels][3] u64 | table [kStripPixels] {place, samples}
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
    return for_bvh_pool_slots(slots, [=](auto sl) { return adapt_pool_kernel_<decltype(sl)::value>(hosek); });
}

// The render stage of a pooled step: grid_blocks blocks of kBvhPoolThreads, whose waves stride over the units of 16 list entries; a.lds_bytes =
// mirt_adapt_pool_plan's bytes per block, a.bvh_stack_entries its stack entries
hipError_t launch_adapt_pixels_pool(const RenderArgs& a, void* d_recs, const uint32_t* d_list, const uint32_t* d_count, uint32_t grid_blocks, uint32_t slots, bool hosek,
                                    hipStream_t stream)
{
    const AdaptPoolKernel k = adapt_pool_kernel(slots, hosek);
    if (!k) return hipErrorInvalidValue;
    return launch_with_lds(k, dim3(grid_blocks), dim3(kBvhPoolThreads), a, LaunchOn(stream), static_cast<adapt_u4*>(d_recs), d_list, d_count);
}
