/*
 * mirt_oracle_resolve.h — the path-traced mode's per-sample fixed-point conversion (S2) and the resolve of one
 * exact 64-bit channel sum to an 8-bit code (S5): mean -> uncharted2 (wgsl:83-103) -> sRGB OETF -> round to nearest.
 *
 * TEST INFRASTRUCTURE ONLY (see mirt_oracle.h).  A header of its own so that the CPU oracle, its host exports and the
 * test-only device probe (mirt_math_probe.hip) evaluate the same sequence.
 */
#ifndef MIRT_ORACLE_RESOLVE_H
#define MIRT_ORACLE_RESOLVE_H

#include <stdint.h>

#include "../include/mirt.h"
#include "mirt_oracle_math.h"

/* radiance -> unsigned fixed point, 2^-20 units, clamped to [0, 4096) */
static inline uint32_t to_fixed(float c)
{
    if (!(c > 0.0f)) return 0;                       /* negatives and NaN */
    float s = c * 1048576.0f;
    if (s >= 4294967040.0f) s = 4294967040.0f;        /* largest f32 below 2^32 */
    return (uint32_t)s;
}

static inline float uncharted2_tonemap(float x)
{
    const float A = 0.15f, B = 0.50f, CB = 0.05f, DE = 0.004f, DF = 0.06f;
    const float EF = 0.02f / 0.30f;
    float num = MFMA(x, MFMA(A, x, CB), DE);
    float den = MFMA(x, MFMA(A, x, B), DF);
    return num / den - EF;
}

static inline float uncharted2(float x)
{
    float curr = uncharted2_tonemap(0.246f * x);
    float white = 1.0f / uncharted2_tonemap(11.2f);
    return white * curr;
}

static inline float srgb_oetf(float x)
{
    if (!(x > 0.0031308f)) return 12.92f * x;
    return MFMA(1.055f, om_pow_pos(x, 0.41666666f), -0.055f);
}

static inline uint8_t quantise(float x)
{
    if (!(x > 0.0f)) return 0;
    if (x > 1.0f) x = 1.0f;
    return (uint8_t)MFMA(x, 255.0f, 0.5f);
}

/* one channel: the sum of n_samples fixed-point samples -> its 8-bit code.  The mean is sum / (n * 2^20) in double,
 * rounded once to float. */
static inline uint32_t om_resolve_channel(uint64_t sum, uint32_t n_samples, uint32_t flags)
{
    double denom = (double)n_samples * 1048576.0;
    float m = (float)((double)sum / denom);
    if (!(flags & MIRT_FLAG_NO_TONEMAP)) m = uncharted2(m);
    if (!(flags & MIRT_FLAG_NO_SRGB)) m = srgb_oetf(m);
    return quantise(m);
}

#endif /* MIRT_ORACLE_RESOLVE_H */
