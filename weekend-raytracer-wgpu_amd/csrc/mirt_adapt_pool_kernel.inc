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
// The kernel's text is mirt_adapt_pool_text.inc, included twice: a step of a RUN (DESIGN.md 10.14) launches
// adapt_pixels_pool_run_kernel, the same text with spp read from the word behind the count -- a unit then holds up to 16 x 2^24 items,
// which the 32-bit item counters hold -- in the same geometries, on the same plan.

// PoolHbmState's state word with the parity of the path's sample index in a bit that struct leaves free (25 .. 30)
struct AdaptPoolState {
    static constexpr uint32_t kEvenShift = 25;
    static_assert(kEvenShift > PoolHbmState::kMissShift && kEvenShift < PoolHbmState::kHitShift, "a bit PoolHbmState::flags never sets");
    static MIRT_DEV uint32_t flags(uint32_t r, uint32_t bounce, uint32_t miss, uint32_t even) { return PoolHbmState::flags(r, bounce, miss) | (even << kEvenShift); }
    static MIRT_DEV uint32_t even(uint32_t fl) { return (fl >> kEvenShift) & 1u; }
};

// adapt_pixels_pool_kernel (a step: spp is the launch's) and adapt_pixels_pool_run_kernel (a step of a run, DESIGN.md 10.14: spp is the word
// behind the count, wave-uniform), one text
#define MIRT_ADAPT_POOL_KERNEL adapt_pixels_pool_kernel
#define MIRT_ADAPT_RUN 0
#include "mirt_adapt_pool_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_POOL_KERNEL
#define MIRT_ADAPT_POOL_KERNEL adapt_pixels_pool_run_kernel
#define MIRT_ADAPT_RUN 1
#include "mirt_adapt_pool_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_POOL_KERNEL

// ---- one build per geometry of kBvhPoolSlotChoices (the pooled HBM render's table) x HOSEK ----
static QueryKernel adapt_pool_kernel(const QueryPlan& p)
{
    if (p.threads != kBvhPoolThreads || p.min_waves != kBvhPoolMinWaves) return nullptr;      // not a geometry of plan_bvh_pool
    return for_bvh_pool_slots(p.slots, [&](auto sl) -> QueryKernel {
        constexpr uint32_t T = kBvhPoolThreads, SL = decltype(sl)::value, MW = kBvhPoolMinWaves;
        if (p.run) return with_bools<QueryKernel>([](auto H) { return kernel_handle(adapt_pixels_pool_run_kernel<T, SL, MW, H.value>); }, p.hosek);
        return with_bools<QueryKernel>([](auto H) { return kernel_handle(adapt_pixels_pool_kernel<T, SL, MW, H.value>); }, p.hosek);
    });
}
