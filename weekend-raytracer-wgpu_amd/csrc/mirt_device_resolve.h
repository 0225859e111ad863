// mirt_device_resolve.h — the path-traced mode's per-sample fixed-point conversion and the resolve of an exact 64-bit
// sum to one 8-bit code: mean -> uncharted2 (wgsl:83-103) -> sRGB OETF -> round to nearest.  Included by
// mirt_kernels.hip, so the exact and the fast build both compile it with their own elementary functions.
#pragma once

#include "../../include/mirt.h"
#include "mirt_device_math.h"

namespace mirt {
namespace MIRT_KNS {

MIRT_DEV uint32_t to_fixed(float c)          // 2^-20 units, clamped to [0, 4096)
{
    const float p = (c > 0.0f) ? c : 0.0f;                  // NaN and negatives -> 0 (select, no branch)
    const float s = __builtin_fminf(p * 1048576.0f, 4294967040.0f);    // p is never NaN here: one v_min_f32
    return (uint32_t)s;
}

MIRT_DEV float uncharted2_tonemap(float x)   // wgsl:94-103
{
    const float A_ = 0.15f, B_ = 0.50f, CB = 0.05f, DE = 0.004f, DF = 0.06f;
    const float EF = 0.02f / 0.30f;
    const float num = fma_(x, fma_(A_, x, CB), DE);
    const float den = fma_(x, fma_(A_, x, B_), DF);
    return num / den - EF;
}

MIRT_DEV uint32_t resolve_channel(unsigned long long sum, uint32_t n_samples, uint32_t flags)
{
    // mean = sum / (n * 2^20), in double, rounded once to float (mirt-math v1's definition of the mean).  A power-of-two sample count -- the reference adds
    // 2 per frame -- makes the divisor a power of two: the quotient is an exact scaling of (double)sum (one v_ldexp_f64), without the f64
    // division (about 20 of the ~105 instructions of a channel).  Wave-uniform choice; n_samples >= 1.
    const double denom = (double)n_samples * 1048576.0;
    float m;
    if ((n_samples & (n_samples - 1u)) == 0u) m = (float)__builtin_ldexp((double)sum, -(int)(20u + (uint32_t)__builtin_ctz(n_samples)));
    else m = (float)((double)sum / denom);
    if (!(flags & MIRT_FLAG_NO_TONEMAP)) {   // uncharted2 wgsl:83-92
        const float curr = uncharted2_tonemap(0.246f * m);
        const float white = rcp_(uncharted2_tonemap(11.2f));
        m = white * curr;
    }
    if (!(flags & MIRT_FLAG_NO_SRGB))        // the Bgra8UnormSrgb surface's transfer curve
        m = (m > 0.0031308f) ? fma_(1.055f, pow_pos(m, 0.41666666f), -0.055f) : 12.92f * m;
    if (!(m > 0.0f)) return 0u;
    m = (m > 1.0f) ? 1.0f : m;
    return (uint32_t)fma_(m, 255.0f, 0.5f);
}

}  // namespace MIRT_KNS
}  // namespace mirt
