// mirt_adapt_scan_text.inc -- the scan stage of an adaptive step, as TEXT: mirt_adapt_kernel.inc includes it twice (the scan behind a
// MIRT_DEV function of both kernels cost adapt_scan_kernel two VGPRs; as text it is token for token what it was).
//   MIRT_ADAPT_RUN 0   adapt_scan_kernel: head[0] = the step's count; the 64-bit word at head + 2 = samples added since the reset
//   MIRT_ADAPT_RUN 1   adapt_scan_run_kernel, a step of a RUN (mirt_ctx_adapt_run_device; DESIGN.md 10.14): thread 0 also chooses the step's
//                      sample count from the count it has just summed -- adapt_run_spp of mirt_adapt_rule.h, the function
//                      mirt_adapt_run_spp runs on the host -- and writes it into the head's free word, head[1], where
//                      adapt_pixels_run_kernel / adapt_pixels_pool_run_kernel read it, and {count, spp} into this step's entry of the run
//                      log.  Plain stores of one thread; the stream orders them before the render stage.
#if MIRT_ADAPT_RUN
__global__ __launch_bounds__(kAdaptScanThreads) void adapt_scan_run_kernel(uint32_t* block_counts, uint32_t n_blocks, uint32_t* head, uint32_t base_spp,
                                                                           uint32_t min_items, uint32_t cap_spp, uint2* log_entry)
#else
__global__ __launch_bounds__(kAdaptScanThreads) void adapt_scan_kernel(uint32_t* block_counts, uint32_t n_blocks, uint32_t* head, uint32_t spp)
#endif
{
    __shared__ uint32_t wave_total[kAdaptScanThreads / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += kAdaptScanThreads) {      // (base stays below 2^24: at most 2^32 / 256 blocks)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_counts[i] : 0u;
        uint32_t incl = v;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kAdaptScanThreads / 64u; ++w) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        if (i < n_blocks) block_counts[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
#if MIRT_ADAPT_RUN
        const uint32_t spp = adapt_run_spp(carry, base_spp, min_items, cap_spp);
        head[1] = spp;
        *log_entry = make_uint2(carry, spp);
#endif
        head[0] = carry;
        unsigned long long* total = reinterpret_cast<unsigned long long*>(head + 2);
        *total += (unsigned long long)carry * spp;
    }
}
