// mirt_radiance_pool_kernel.inc -- the pooled schedule for radiance queries (MIRT_RADIANCE_POOL on mirt_ctx_trace_radiance*; DESIGN.md
// 10.11).  Included once by mirt_kernels.hip behind mirt_radiance_kernel.inc, exact build only: no fast_build:: copy, no counting build.
//
// The schedule of radiance_rays_pool_kernel<THREADS, SLOTS, MINW, HOSEK, SORTED> is mirt_pool_hbm_schedule.inc; this file holds what is
// the kernel's own:
//   * a unit is kStripPixels = 16 consecutive SLOTS OF THE BATCH, not pixels: slot k is ray k, or ray order[k] when SORTED (the
//     permutation ray_sort_order left in device memory).  RenderArgs.n_units = ceil(n_rays / 16), RenderArgs.width = n_rays.  A unit's
//     work items are unit_rays x spp, item -> (sample = item / unit_rays, r = item % unit_rays); r takes the place of the pixel in
//     PoolHbmState::flags and in L_acc.  There are no strip levels and no camera.
//   * OP_GEN loads the item's ray from memory as radiance_rays_kernel does (two 16-byte loads: {origin, stream} {direction, _pad}), seeds
//     the stream of (stream, sample) and skips the four draws of a primary ray.  A lane without an item loads nothing.
//   * there is no dispenser: a wave takes unit first_unit(), then every grid_waves-th behind it.  The epilogue writes MirtRadiance
//     records through mirt_radiance_record_text.inc, the text the per-lane kernels include: no resolve, no counters.
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

#define MIRT_POOL_HBM_PART 1           // every slot into the OP_GEN queue, sums zeroed; tail[], next_item and the loop-carried state
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART

        for (;;) {
            if (!ff) {
#define MIRT_POOL_HBM_PART 2           // pick the deepest queue (or leave the loop), pop, gather; fl = the state word
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
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
#define MIRT_POOL_HBM_PART 3           // sphere and material from device memory, shade_by_id
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
            }

#define MIRT_POOL_HBM_STATE_WORD St::flags(pix, bounce, miss)
#define MIRT_POOL_HBM_PART 4           // bounce limit, nearest_hit_bvh, classification, fast-forward, store, push
#include "mirt_pool_hbm_schedule.inc"
#undef MIRT_POOL_HBM_PART
#undef MIRT_POOL_HBM_STATE_WORD
        }

        // ---- unit finished: lane r < unit_rays owns the record of the unit's r-th slot ----
        if (lane < unit_rays) {
            const RenderArgs& AS = per_strip_args();
            uint64_t i = base_slot + lane;
            if constexpr (SORTED) i = order[i];
            unsigned long long acc_r = L_acc[lane * 3 + 0], acc_g = L_acc[lane * 3 + 1], acc_b = L_acc[lane * 3 + 2];
#define MIRT_RADIANCE_ARGS AS
#include "mirt_radiance_record_text.inc"
#undef MIRT_RADIANCE_ARGS
        }
    }
}

// ---- one build per geometry of kBvhPoolSlotChoices (the pooled HBM render's table) x HOSEK x SORTED ----
static QueryKernel radiance_pool_kernel(const QueryPlan& p)
{
    if (p.threads != kBvhPoolThreads || p.min_waves != kBvhPoolMinWaves) return nullptr;      // not a geometry of plan_bvh_pool
    return for_bvh_pool_slots(p.slots, [&](auto sl) -> QueryKernel {
        constexpr uint32_t T = kBvhPoolThreads, SL = decltype(sl)::value, MW = kBvhPoolMinWaves;
        return with_bools<QueryKernel>([](auto H, auto S) { return kernel_handle(radiance_rays_pool_kernel<T, SL, MW, H.value, S.value>); }, p.hosek, p.sorted);
    });
}
