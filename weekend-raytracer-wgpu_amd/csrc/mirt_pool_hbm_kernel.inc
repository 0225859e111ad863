// mirt_pool_hbm_kernel.inc -- the text of the pooled path-traced kernel of MIRT_SCENE_HBM scenes (MIRT_FLAG_KERNEL_POOL on such a
// scene; DESIGN.md 10.6).  mirt_kernels.hip includes it twice:
//   MIRT_POOL_HBM_KERNEL_NAME = render_pt_pool_hbm_kernel,       MIRT_POOL_HBM_KERNEL_FRAME = false
//   MIRT_POOL_HBM_KERNEL_NAME = render_pt_pool_hbm_frame_kernel, MIRT_POOL_HBM_KERNEL_FRAME = true   (the progressive-frame build)
// The schedule is mirt_pool_hbm_schedule.inc; this file holds what is the kernel's own:
//   * a unit is a strip of 16 pixels (8, 4, 2, 1 in the guided levels) x spp work items, handed out by mirt_pool_kernel.inc's dispenser;
//     OP_GEN turns an item into a camera ray with the camera re-read from LDS.
//   * behind the block's pools every wave has 64 traversal stacks of RenderArgs.bvh_stack_entries node references -- the depth of the
//     RESIDENT tree, not MIRT_BVH_MAX_DEPTH: 256 x depth bytes per wave (mirt_bvh_pool_plan).
//   * the three epilogues of mirt_pool_kernel.inc (image, sums, progressive frame), and the only counting build of the schedule: the
//     steps of a wave are counted here, between the parts, the traced lanes in the shared tail.
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
