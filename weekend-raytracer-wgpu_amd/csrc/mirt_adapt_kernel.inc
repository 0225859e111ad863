// mirt_adapt_kernel.inc -- adaptive sampling for progressive frames of a resident MIRT_SCENE_HBM scene (mirt_ctx_adapt_*; include/mirt.h,
// DESIGN.md 10.12).  Included once by mirt_kernels.hip behind mirt_radiance_pool_kernel.inc, exact build only: there is no fast_build::
// copy, no counting build and no dispenser.  The context keeps one MirtAdaptPixel per pixel (64 bytes: three u64 sums, the three sums of
// the even-indexed samples, samples, pads), 16-byte aligned: a record is four 16-byte accesses {sum0, sum1} {sum2, even0} {even1, even2}
// {samples, 0, 0, 0}.
//
// A step is four kernels on one stream:
//   adapt_select_kernel   lane = record: three 16-byte loads of the sums and one of the count, then the rule of mirt_adapt_rule.h (the
//                         function mirt_adapt_active runs on the host: 128-bit products).  One flag byte per record, and per block of
//                         kAdaptSelectThreads records the number of active ones.
//   adapt_scan_kernel     ONE block: the exclusive prefix sums of the block counts, in place, 1024 at a time with a running carry; thread 0
//                         then writes the step's count into the head word and adds count x spp to the 64-bit sample counter behind it.
//   adapt_compact_kernel  lane = record again: a record's place in the list is its block's offset + the active records before it in the
//                         block (ballot + popcount within the wave, the waves' totals through LDS), so the list is ASCENDING by
//                         construction and the same whatever order the blocks run in.
//   adapt_pixels_kernel<HOSEK, BVH>   the shape of radiance_rays_kernel: lane = list entry, 64 consecutive entries per wave, ONE wave per
//                         block, LDS = stage_scene's image without the tables (the launch's camera, the sky blob) | the wave's traversal
//                         stacks, 8 KB.  The grid is sized for ALL pixels (the host does not know the count): the count is read as a
//                         wave-uniform word before anything is staged and blocks beyond it return at once.  A lane loads its record,
//                         takes spp samples n .. n + spp - 1 of ITS pixel's stream -- generate_primary with the camera from LDS as in
//                         the strip body, for the pixel's absolute (x, y), then path_radiance with the source render_pt_hbm_kernel gives
//                         it -- adds every sample's three fixed-point values to `sum` and those of even-indexed samples to `even`, and
//                         writes the record back with four 16-byte stores.  Lanes of the last wave beyond the count load nothing, take
//                         part in the wave's loops with their tests masked off and store nothing.
//   adapt_resolve_kernel  per pixel resolve_channel(sum[k], samples, flags); samples == 0: black, A = 255.
//
// A step of a RUN (mirt_ctx_adapt_run_device; DESIGN.md 10.14) is the same four kernels with two of them in a second build: the scan
// stage's thread 0 also chooses the step's sample count from the count it has just summed (adapt_run_spp of mirt_adapt_rule.h), writes
// it into head[1] and {count, spp} into the run log (adapt_scan_run_kernel), and the render stage reads that word next to the count in
// the place of A.spp (adapt_pixels_run_kernel<HOSEK, BVH>).  The second builds share their TEXT with the first
// (mirt_adapt_scan_text.inc, mirt_adapt_pixels_text.inc), so a step's kernels keep their names and their code.

typedef uint32_t adapt_u4 __attribute__((ext_vector_type(4)));        // a record's quarter, 16-byte aligned (the buffer is the context's own)

constexpr uint32_t kAdaptSelectThreads = 256;       // adapt_select_kernel / adapt_compact_kernel: records per block
constexpr uint32_t kAdaptScanThreads = 1024;

MIRT_DEV unsigned long long adapt_u64(uint32_t lo, uint32_t hi) { return (unsigned long long)lo | ((unsigned long long)hi << 32); }

__global__ __launch_bounds__(kAdaptSelectThreads) void adapt_select_kernel(const adapt_u4* recs, uint32_t n, MirtAdaptParams P, unsigned char* flags,
                                                                           uint32_t* block_counts)
{
    __shared__ uint32_t wave_count[kAdaptSelectThreads / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * kAdaptSelectThreads + threadIdx.x;
    bool active = false;
    if (i < n) {
        const adapt_u4 q0 = recs[4u * i], q1 = recs[4u * i + 1u], q2 = recs[4u * i + 2u], q3 = recs[4u * i + 3u];
        const uint64_t sum[3] = { adapt_u64(q0.x, q0.y), adapt_u64(q0.z, q0.w), adapt_u64(q1.x, q1.y) };
        const uint64_t even[3] = { adapt_u64(q1.z, q1.w), adapt_u64(q2.x, q2.y), adapt_u64(q2.z, q2.w) };
        active = adapt_active(sum, even, q3.x, P);
        flags[i] = active ? 1u : 0u;
    }
    const unsigned long long mask = ballot_(active);
    if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kAdaptSelectThreads / 64u; ++w) t += wave_count[w];
        block_counts[blockIdx.x] = t;
    }
}

// adapt_scan_kernel (a step: spp is the launch's) and adapt_scan_run_kernel (a step of a run: thread 0 chooses spp and logs it), one text
#define MIRT_ADAPT_RUN 0
#include "mirt_adapt_scan_text.inc"
#undef MIRT_ADAPT_RUN
#define MIRT_ADAPT_RUN 1
#include "mirt_adapt_scan_text.inc"
#undef MIRT_ADAPT_RUN

__global__ __launch_bounds__(kAdaptSelectThreads) void adapt_compact_kernel(const unsigned char* flags, uint32_t n, const uint32_t* block_offsets, uint32_t* list)
{
    __shared__ uint32_t wave_count[kAdaptSelectThreads / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * kAdaptSelectThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool active = i < n && flags[i] != 0u;
    const unsigned long long mask = ballot_(active);
    if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (active) {
        uint32_t at = block_offsets[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) at += wave_count[w];
        list[at] = (uint32_t)i;          // at < the step's count <= n: the offsets are the prefix sums of these very flags
    }
}

// adapt_pixels_kernel<HOSEK, BVH> (a step: spp is the launch's) and adapt_pixels_run_kernel<HOSEK, BVH> (a step of a run: spp is the word
// behind the count), one text
#define MIRT_ADAPT_PIXELS_KERNEL adapt_pixels_kernel
#define MIRT_ADAPT_RUN 0
#include "mirt_adapt_pixels_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_PIXELS_KERNEL
#define MIRT_ADAPT_PIXELS_KERNEL adapt_pixels_run_kernel
#define MIRT_ADAPT_RUN 1
#include "mirt_adapt_pixels_text.inc"
#undef MIRT_ADAPT_RUN
#undef MIRT_ADAPT_PIXELS_KERNEL

__global__ __launch_bounds__(256) void adapt_resolve_kernel(const adapt_u4* recs, uint32_t* out, uint64_t n_pixels, uint32_t flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += (uint64_t)gridDim.x * blockDim.x) {
        const adapt_u4 q0 = recs[4u * i], q1 = recs[4u * i + 1u], q3 = recs[4u * i + 3u];
        const uint32_t n = q3.x;
        uint32_t rgba = 0xff000000u;
        if (n != 0u)
            rgba = pack_rgba(resolve_channel(adapt_u64(q0.x, q0.y), n, flags), resolve_channel(adapt_u64(q0.z, q0.w), n, flags),
                             resolve_channel(adapt_u64(q1.x, q1.y), n, flags));
        out[i] = rgba;
    }
}

// The select stage of a step for n >= 1 records at d_recs: flags [n] bytes, block counts [ceil(n / 256)] words, the list [n] words and the
// head {count, -, 64-bit sample counter} are the context's (16-byte aligned head and records).
hipError_t launch_adapt_select(const void* d_recs, uint32_t n, const MirtAdaptParams& adapt, uint32_t spp, unsigned char* d_flags, uint32_t* d_block_counts,
                               uint32_t* d_list, uint32_t* d_head, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)n + kAdaptSelectThreads - 1u) / kAdaptSelectThreads);
    hipLaunchKernelGGL(adapt_select_kernel, dim3(blocks), dim3(kAdaptSelectThreads), 0, stream, static_cast<const adapt_u4*>(d_recs), n, adapt, d_flags, d_block_counts);
    hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(kAdaptScanThreads), 0, stream, d_block_counts, blocks, d_head, spp);
    hipLaunchKernelGGL(adapt_compact_kernel, dim3(blocks), dim3(kAdaptSelectThreads), 0, stream, d_flags, n, d_block_counts, d_list);
    return hipGetLastError();
}

// The select stage of a step of a run: the same three kernels with adapt_scan_run_kernel in the middle, which derives the step's sample
// count (base_spp, min_items, cap_spp: adapt_run_spp's arguments) and writes {count, spp} to d_log_entry, 8-byte aligned.
hipError_t launch_adapt_select_run(const void* d_recs, uint32_t n, const MirtAdaptParams& adapt, uint32_t base_spp, uint32_t min_items, uint32_t cap_spp,
                                   unsigned char* d_flags, uint32_t* d_block_counts, uint32_t* d_list, uint32_t* d_head, void* d_log_entry, hipStream_t stream)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)n + kAdaptSelectThreads - 1u) / kAdaptSelectThreads);
    hipLaunchKernelGGL(adapt_select_kernel, dim3(blocks), dim3(kAdaptSelectThreads), 0, stream, static_cast<const adapt_u4*>(d_recs), n, adapt, d_flags, d_block_counts);
    hipLaunchKernelGGL(adapt_scan_run_kernel, dim3(1), dim3(kAdaptScanThreads), 0, stream, d_block_counts, blocks, d_head, base_spp, min_items, cap_spp,
                       static_cast<uint2*>(d_log_entry));
    hipLaunchKernelGGL(adapt_compact_kernel, dim3(blocks), dim3(kAdaptSelectThreads), 0, stream, d_flags, n, d_block_counts, d_list);
    return hipGetLastError();
}

// The render stage (run: adapt_pixels_run_kernel, which takes the step's sample count from the word behind the count and not from RenderArgs.spp)
static QueryKernel adapt_kernel(const QueryPlan& p)
{
    if (!p.run) return with_bools<QueryKernel>([](auto H, auto B) { return kernel_handle(adapt_pixels_kernel<H.value, B.value>); }, p.hosek, p.bvh);
    return with_bools<QueryKernel>([](auto H, auto B) { return kernel_handle(adapt_pixels_run_kernel<H.value, B.value>); }, p.hosek, p.bvh);
}

hipError_t launch_adapt_resolve(const void* d_recs, uint32_t* out, uint64_t n_pixels, uint32_t flags, hipStream_t stream)
{
    uint32_t blocks = (uint32_t)((n_pixels + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(adapt_resolve_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<const adapt_u4*>(d_recs), out, n_pixels, flags);
    return hipGetLastError();
}
