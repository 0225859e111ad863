// mirt_feature_item_text.inc -- one pixel of a feature frame from its centre ray to its record, as TEXT: included by feature_frame_kernel
// and feature_frame_lds_kernel with `i`, `alive`, `x`, `y`, C, `work` and `out` in scope.
//   MIRT_FEATURE_NEAREST   the nearest-hit expression over (ro, rd, alive, closest, work)
//   MIRT_FEATURE_OF_HIT    the call that fills (hn, al) from (best, closest, ro, rd): feature_of_hit with the layout's tables
    // the centre ray
#include "mirt_centre_ray_text.inc"
    float closest;
    int best = MIRT_FEATURE_NEAREST;
    const uint32_t sphere = best >= 0 ? (uint32_t)best : kTraceMiss;
    const float t = best >= 0 ? closest : 0.0f;

    // the sample set: wave-uniform trip count; for spp == 0 the one sample is the centre ray and its hit above
    f3 sum_n = mk(0, 0, 0), sum_a = mk(0, 0, 0);
    const uint32_t n = A.spp ? A.spp : 1u;
    Rng rng;
    rng.state = 0u;
    for (uint32_t s = 0; s < n; ++s) {
        if (A.spp != 0u) {
            generate_primary(A, C, x, y, A.sample_begin + s, rng, ro, rd);
            best = MIRT_FEATURE_NEAREST;
        }
        if (alive && best >= 0) {
            f3 hn, al;
            MIRT_FEATURE_OF_HIT;
            sum_n = sum_n + hn;
            sum_a = sum_a + al;
        }
    }
    if (alive) {
        const float fn = (float)n;
        out[2u * i] = trace_u4{ bits(sum_a.x / fn), bits(sum_a.y / fn), bits(sum_a.z / fn), bits(t) };
        out[2u * i + 1u] = trace_u4{ bits(sum_n.x / fn), bits(sum_n.y / fn), bits(sum_n.z / fn), sphere };
    }
