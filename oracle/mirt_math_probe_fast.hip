// mirt_math_probe_fast.hip — TEST INFRASTRUCTURE ONLY: mirt_math_probe.hip compiled a second time with the product's
// FAST_FLAGS, into namespace mirt::fast_build, the way csrc/mirt_kernels_fast.hip compiles mirt_kernels.hip: the
// elementary functions and the resolve of the opt-in fast-math build (MIRT_FLAG_FAST_MATH).
#define MIRT_FAST_MATH 1
#define MIRT_KNS fast_build
#include "mirt_math_probe.hip"
