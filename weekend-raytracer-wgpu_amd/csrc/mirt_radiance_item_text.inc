// mirt_radiance_item_text.inc -- one ray of a radiance query, as TEXT: included by radiance_rays_kernel and radiance_rays_sorted_kernel
// (through mirt_radiance_ray_body.inc) and by radiance_rays_lds_kernel, with `i`, `alive`, `lane`, `work`, S and G in scope.
//   MIRT_RADIANCE_GRID, MIRT_RADIANCE_SRC   path_radiance's GRID and SRC template arguments
//   MIRT_RADIANCE_STACK                     its traversal stack pointer
// The stream is seeded from the ray's `stream` word, the four draws of a primary ray are skipped, and the three sums of
// to_fixed(radiance) stay per lane as 64-bit integers until mirt_radiance_record_text.inc stores them.
    trace_u4 r0 = { 0u, 0u, 0u, 0u }, r1 = { 0u, 0u, 0u, 0u };
    if (alive) { r0 = rays[2u * i]; r1 = rays[2u * i + 1u]; }          // {origin, stream} {direction, _pad}
    const f3 ro = mk(from_bits(r0.x), from_bits(r0.y), from_bits(r0.z));
    const f3 rd = mk(from_bits(r1.x), from_bits(r1.y), from_bits(r1.z));
    const uint32_t stream = r0.w;

    unsigned long long acc_r = 0, acc_g = 0, acc_b = 0;
    for (uint32_t s = 0; s < A.spp; ++s) {
        Rng rng;
        // generate_primary's seed with `stream` for the pixel index, then the two jitter and the two lens draws of a primary ray
        rng.state = jenkins_hash((stream ^ jenkins_hash(A.sample_begin + s + 1u)) ^ A.seed_mix);
        rng.skip(); rng.skip(); rng.skip(); rng.skip();
        const f3 c = path_radiance<false, HOSEK, MIRT_RADIANCE_GRID, MIRT_RADIANCE_SRC>(A, S, G, alive, rng, ro, rd, work, lane, nullptr, kNoCand, MIRT_RADIANCE_STACK);
        acc_r += to_fixed(c.x);
        acc_g += to_fixed(c.y);
        acc_b += to_fixed(c.z);
    }
    if (alive) {
#define MIRT_RADIANCE_ARGS A
#include "mirt_radiance_record_text.inc"
#undef MIRT_RADIANCE_ARGS
    }
