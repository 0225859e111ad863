// mirt_math_probe.hip — TEST INFRASTRUCTURE ONLY: the device side of tests/test_gpu_math_exhaustive.py and
// tests/test_gpu_resolve.py.  The product never loads or links it.
//
// It evaluates the product's elementary functions (csrc/mirt_device_math.h) and its resolve (csrc/mirt_device_resolve.h)
// on given inputs, and compares them ON THE DEVICE with the oracle's sequences (mirt_oracle_math.h,
// mirt_oracle_resolve.h), which are compiled for gfx950 here too (force_cuda_host_device), over whole ranges of bit
// patterns.  This translation unit is compiled with the product's FLAGS (csrc/Makefile); mirt_math_probe_fast.hip
// compiles it a second time with FAST_FLAGS, the way csrc/mirt_kernels_fast.hip does, for the fast build's functions.
//
// Every entry point takes host pointers, runs on a stream of its own and synchronises before it returns.
// Two results are equal when their bits are equal or when both are NaN (NaN payloads are not specified).
#include <string.h>      // before the pragma below: glibc's memcpy / memset must stay host functions
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../weekend-raytracer-wgpu_amd/csrc/mirt_device_math.h"
#include "../weekend-raytracer-wgpu_amd/csrc/mirt_device_resolve.h"

// function ids of mprobe_eval / mprobe_sweep (tests/math_probe.py mirrors them)
enum MprobeFn : int {
    MP_SINCOS = 0,          // a -> (sin, cos)
    MP_SINCOS_SMALL = 1,    // a -> (sin, cos), |a| <= 2^20
    MP_SIN_SIGN = 2,        // a -> int {-1, 0, +1}
    MP_SIN_SIGN_BITS = 3,   // a -> sin_sign_bits decoded to {-1, 0, +1}
    MP_SIN_PRODUCT_NEG = 4, // (a, b, c) -> 0 / 1
    MP_ACOS = 5,            // a
    MP_ATAN2 = 6,           // (a = y, b = x)
    MP_LOG2 = 7,
    MP_EXP2 = 8,
    MP_EXP = 9,
    MP_POW_POS = 10,        // (a = x, b = y)
    MP_POW_UNIT = 11,       // (a = x, b = y), x = 0 or 2^-32 <= x <= 1, 0 < y <= 1
    MP_RCP_IN_RANGE = 12,   // 2^-100 <= |a| <= 2^100
    MP_SQRT_UNIT_WHERE = 13,// sqrt_unit_where(a, true), 0 < a <= 1
    MP_TO_FIXED = 14,       // a -> uint32
    MP_N_FN = 15,
};
// sweep-only ids: the sweep's pattern is one operand, the params are the other
enum MprobeSweepFn : int {
    MP_SW_ATAN2_Y = 100,    // pattern = y, x = each param
    MP_SW_ATAN2_X = 101,    // pattern = x, y = each param
    MP_SW_POW_PAIRS = 102,  // index -> a seeded (x, y) pair (params[0] = seed)
    MP_SW_SIN_PRODUCT = 103,// index -> a seeded triple; a quarter of the components are drawn from the params
};
enum MprobeBuild : int { MP_EXACT = 0, MP_FAST = 1, MP_ORACLE = 2 };

namespace mirt {
namespace MIRT_KNS {

// one product function; results as bit patterns
MIRT_DEV void probe_product(int fn, float a, float b, float c, uint32_t& o0, uint32_t& o1)
{
    o1 = 0u;
    switch (fn) {
    case MP_SINCOS: { const SinCos r = sincos_(a); o0 = bits(r.s); o1 = bits(r.c); break; }
    case MP_SINCOS_SMALL: { const SinCos r = sincos_small(a); o0 = bits(r.s); o1 = bits(r.c); break; }
    case MP_SIN_SIGN: o0 = (uint32_t)sin_sign(a); break;
    case MP_SIN_SIGN_BITS: {
        uint32_t neg;
        const uint32_t z = sin_sign_bits(a, neg);
        o0 = (z == 0u) ? 0u : ((neg & 1u) ? (uint32_t)-1 : 1u);
        o1 = z;
        break;
    }
    case MP_SIN_PRODUCT_NEG: o0 = sin_product_negative(a, b, c) ? 1u : 0u; break;
    case MP_ACOS: o0 = bits(acos_(a)); break;
    case MP_ATAN2: o0 = bits(atan2_(a, b)); break;
    case MP_LOG2: o0 = bits(log2_(a)); break;
    case MP_EXP2: o0 = bits(exp2_(a)); break;
    case MP_EXP: o0 = bits(exp_(a)); break;
    case MP_POW_POS: o0 = bits(pow_pos(a, b)); break;
    case MP_POW_UNIT: o0 = bits(pow_unit(a, b)); break;
    case MP_RCP_IN_RANGE: o0 = bits(rcp_in_range(a)); break;
    case MP_SQRT_UNIT_WHERE: o0 = bits(sqrt_unit_where(a, true)); break;
    case MP_TO_FIXED: o0 = to_fixed(a); break;
    default: o0 = 0xdeadbeefu; break;
    }
}

__global__ __launch_bounds__(256) void probe_eval_kernel(int fn, const float* a, const float* b, const float* c, uint32_t* o0,
                                                         uint32_t* o1, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t r0, r1;
        probe_product(fn, a ? a[i] : 0.0f, b ? b[i] : 0.0f, c ? c[i] : 0.0f, r0, r1);
        o0[i] = r0;
        if (o1) o1[i] = r1;
    }
}

__global__ __launch_bounds__(256) void probe_resolve_kernel(const unsigned long long* sums, uint8_t* out, uint64_t n, uint32_t n_samples,
                                                            uint32_t flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)resolve_channel(sums[i], n_samples, flags);
}

static uint32_t probe_blocks(uint64_t n)
{
    const uint64_t b = (n + 255) / 256;
    return (uint32_t)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

hipError_t probe_launch_eval(int fn, const float* a, const float* b, const float* c, uint32_t* o0, uint32_t* o1, uint64_t n,
                             hipStream_t s)
{
    hipLaunchKernelGGL(probe_eval_kernel, dim3(probe_blocks(n)), dim3(256), 0, s, fn, a, b, c, o0, o1, n);
    return hipGetLastError();
}

hipError_t probe_launch_resolve(const unsigned long long* sums, uint8_t* out, uint64_t n, uint32_t n_samples, uint32_t flags,
                                hipStream_t s)
{
    hipLaunchKernelGGL(probe_resolve_kernel, dim3(probe_blocks(n)), dim3(256), 0, s, sums, out, n, n_samples, flags);
    return hipGetLastError();
}

}  // namespace MIRT_KNS
}  // namespace mirt

#ifndef MIRT_FAST_MATH
// ---------------------------------------------------------------------------------------------------------------------
// exact build only: the oracle's sequences on the device, the sweeps and the C entry points
// ---------------------------------------------------------------------------------------------------------------------
#pragma clang force_cuda_host_device begin
#include "mirt_oracle_math.h"
#include "mirt_oracle_resolve.h"
#pragma clang force_cuda_host_device end

namespace mirt {
namespace fast_build {
hipError_t probe_launch_eval(int fn, const float* a, const float* b, const float* c, uint32_t* o0, uint32_t* o1, uint64_t n,
                             hipStream_t s);
hipError_t probe_launch_resolve(const unsigned long long* sums, uint8_t* out, uint64_t n, uint32_t n_samples, uint32_t flags,
                                hipStream_t s);
}  // namespace fast_build
}  // namespace mirt

namespace {

namespace X = mirt::exact_build;

// the oracle twin of each product function (the specification it must equal bit for bit)
__device__ __forceinline__ void probe_oracle(int fn, float a, float b, float c, uint32_t& o0, uint32_t& o1)
{
    o1 = 0u;
    switch (fn) {
    case MP_SINCOS:
    case MP_SINCOS_SMALL: { float s, co; om_sincos(a, &s, &co); o0 = om_f2u(s); o1 = om_f2u(co); break; }
    case MP_SIN_SIGN:
    case MP_SIN_SIGN_BITS: o0 = (uint32_t)om_sin_sign(a); break;
    case MP_SIN_PRODUCT_NEG: o0 = (om_sin_sign(a) * om_sin_sign(b) * om_sin_sign(c) < 0) ? 1u : 0u; break;
    case MP_ACOS: o0 = om_f2u(om_acos(a)); break;
    case MP_ATAN2: o0 = om_f2u(om_atan2(a, b)); break;
    case MP_LOG2: o0 = om_f2u(om_log2(a)); break;
    case MP_EXP2: o0 = om_f2u(om_exp2(a)); break;
    case MP_EXP: o0 = om_f2u(om_exp(a)); break;
    case MP_POW_POS:
    case MP_POW_UNIT: o0 = om_f2u(om_pow_pos(a, b)); break;
    case MP_RCP_IN_RANGE: o0 = om_f2u(1.0f / a); break;
    case MP_SQRT_UNIT_WHERE: o0 = om_f2u(sqrtf(a)); break;
    case MP_TO_FIXED: o0 = to_fixed(a); break;
    default: o0 = 0xdeadbeefu; break;
    }
}

__device__ __forceinline__ bool is_float_fn(int fn)
{
    return fn != MP_SIN_SIGN && fn != MP_SIN_SIGN_BITS && fn != MP_SIN_PRODUCT_NEG && fn != MP_TO_FIXED;
}

__device__ __forceinline__ bool same_result(int fn, uint32_t p, uint32_t o)
{
    if (p == o) return true;
    const bool pn = (p & 0x7fffffffu) > 0x7f800000u, on = (o & 0x7fffffffu) > 0x7f800000u;
    return is_float_fn(fn) && pn && on;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// a component of a sin_product_negative triple: special values, raw patterns, or |x| < 2^21 with a random exponent
__device__ __forceinline__ float product_component(uint64_t h, const float* special, uint32_t n_special)
{
    const uint32_t sel = (uint32_t)h & 3u;
    const uint32_t hi = (uint32_t)(h >> 32);
    if (sel == 0u && n_special) return special[hi % n_special];
    if (sel == 1u) return __builtin_bit_cast(float, hi);
    const uint32_t e = 103u + (uint32_t)((h >> 2) & 0xffffu) % 46u;           // 2^-24 .. 2^20
    return __builtin_bit_cast(float, (hi & 0x80000000u) | (e << 23) | (hi & 0x007fffffu));
}

// a seeded (x, y) pair for pow_pos: x any non-negative pattern, y half raw patterns and half |y| < 2^4
__device__ __forceinline__ void pow_pair(uint64_t h, float& x, float& y)
{
    x = __builtin_bit_cast(float, (uint32_t)h & 0x7fffffffu);
    const uint32_t hy = (uint32_t)(h >> 32);
    if (hy & 1u) {
        y = __builtin_bit_cast(float, hy);
    } else {
        const uint32_t e = 100u + (hy >> 1) % 31u;                                  // 2^-27 .. 2^3
        y = __builtin_bit_cast(float, (hy & 0x80000000u) | (e << 23) | ((hy >> 3) & 0x007fffffu));
    }
}

// block-wide reduction of (count, count2, min, evaluated, max) and one set of atomics per block
__device__ void sweep_commit(unsigned long long bad, unsigned long long bad2, unsigned long long minbad, unsigned long long done,
                             unsigned long long maxv, unsigned long long* out)
{
    __shared__ unsigned long long r[5][256];
    const uint32_t t = threadIdx.x;
    r[0][t] = bad; r[1][t] = bad2; r[2][t] = minbad; r[3][t] = done; r[4][t] = maxv;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) {
            r[0][t] += r[0][t + s];
            r[1][t] += r[1][t + s];
            r[2][t] = (r[2][t + s] < r[2][t]) ? r[2][t + s] : r[2][t];
            r[3][t] += r[3][t + s];
            r[4][t] = (r[4][t + s] > r[4][t]) ? r[4][t + s] : r[4][t];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (r[0][0]) atomicAdd(&out[0], r[0][0]);
        if (r[1][0]) atomicAdd(&out[1], r[1][0]);
        if (r[2][0] != ~0ull) atomicMin(&out[2], r[2][0]);
        atomicAdd(&out[3], r[3][0]);
        if (r[4][0]) atomicMax(&out[4], r[4][0]);
    }
}

// product vs oracle over the patterns / indices [lo, lo + count); out = {mismatches, -, smallest mismatching index, evaluated}
__global__ __launch_bounds__(256) void sweep_kernel(int fn, uint64_t lo, uint64_t count, const float* params, uint32_t nparams,
                                                    unsigned long long* out)
{
    unsigned long long bad = 0, minbad = ~0ull, done = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t idx = lo + i;
        const float x = __builtin_bit_cast(float, (uint32_t)idx);
        bool ok = true;
        uint32_t p0, p1, q0, q1;
        if (fn == MP_SW_ATAN2_Y || fn == MP_SW_ATAN2_X || fn == MP_POW_POS || fn == MP_POW_UNIT) {
            const int f = (fn == MP_SW_ATAN2_Y || fn == MP_SW_ATAN2_X) ? MP_ATAN2 : fn;
            for (uint32_t j = 0; j < nparams; ++j) {
                const float a = (fn == MP_SW_ATAN2_X) ? params[j] : x;
                const float b = (fn == MP_SW_ATAN2_X) ? x : params[j];
                X::probe_product(f, a, b, 0.0f, p0, p1);
                probe_oracle(f, a, b, 0.0f, q0, q1);
                ok = ok && same_result(f, p0, q0);
                ++done;
            }
        } else if (fn == MP_SW_POW_PAIRS) {
            float a, b;
            pow_pair(splitmix64(idx ^ ((uint64_t)__builtin_bit_cast(uint32_t, params[0]) << 40)), a, b);
            X::probe_product(MP_POW_POS, a, b, 0.0f, p0, p1);
            probe_oracle(MP_POW_POS, a, b, 0.0f, q0, q1);
            ok = same_result(MP_POW_POS, p0, q0);
            ++done;
        } else if (fn == MP_SW_SIN_PRODUCT) {
            const uint64_t h = splitmix64(idx);
            const float a = product_component(h, params, nparams);
            const float b = product_component(splitmix64(h), params, nparams);
            const float c = product_component(splitmix64(h ^ 0x5851f42d4c957f2dull), params, nparams);
            X::probe_product(MP_SIN_PRODUCT_NEG, a, b, c, p0, p1);
            probe_oracle(MP_SIN_PRODUCT_NEG, a, b, c, q0, q1);
            ok = p0 == q0;
            ++done;
        } else {
            X::probe_product(fn, x, 0.0f, 0.0f, p0, p1);
            probe_oracle(fn, x, 0.0f, 0.0f, q0, q1);
            ok = same_result(fn, p0, q0);
            if (fn == MP_SINCOS || fn == MP_SINCOS_SMALL) ok = ok && same_result(fn, p1, q1);
            ++done;
        }
        if (!ok) {
            ++bad;
            minbad = (idx < minbad) ? idx : minbad;
        }
    }
    sweep_commit(bad, 0, minbad, done, 0, out);
}

// the exact resolve vs the oracle's over sums [lo, lo + count) of the range that starts at range_lo, in runs of 64 consecutive sums per thread;
// out = {mismatches, monotonicity violations (code(s + 1) < code(s), both in range), smallest mismatching sum, evaluated,
//        largest drop code(s) - code(s + 1)}
__global__ __launch_bounds__(256) void resolve_sweep_kernel(uint32_t n_samples, uint32_t flags, uint64_t range_lo, uint64_t lo,
                                                            uint64_t count, unsigned long long* out)
{
    constexpr uint64_t kRun = 64;
    const uint64_t runs = (count + kRun - 1) / kRun;
    unsigned long long bad = 0, mono = 0, minbad = ~0ull, done = 0, drop = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s0 = lo + r * kRun;
        const uint64_t s1 = (count - r * kRun < kRun) ? lo + count : s0 + kRun;
        bool have = s0 > range_lo;                     // the pair (s0 - 1, s0) lies in the whole range
        uint32_t prev = have ? X::resolve_channel(s0 - 1, n_samples, flags) : 0u;
        for (uint64_t s = s0; s < s1; ++s) {
            const uint32_t c = X::resolve_channel(s, n_samples, flags);
            const uint32_t o = om_resolve_channel(s, n_samples, flags);
            if (c != o) {
                ++bad;
                minbad = (s < minbad) ? s : minbad;
            }
            if (have && c < prev) {
                ++mono;
                drop = (prev - c > drop) ? prev - c : drop;
            }
            prev = c;
            have = true;
            ++done;
        }
    }
    sweep_commit(bad, mono, minbad, done, drop, out);
}

__global__ __launch_bounds__(256) void oracle_eval_kernel(int fn, const float* a, const float* b, const float* c, uint32_t* o0,
                                                          uint32_t* o1, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t r0, r1;
        probe_oracle(fn, a ? a[i] : 0.0f, b ? b[i] : 0.0f, c ? c[i] : 0.0f, r0, r1);
        o0[i] = r0;
        if (o1) o1[i] = r1;
    }
}

__global__ __launch_bounds__(256) void oracle_resolve_kernel(const unsigned long long* sums, uint8_t* out, uint64_t n, uint32_t n_samples,
                                                             uint32_t flags)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)om_resolve_channel(sums[i], n_samples, flags);
}

// device buffers and a stream of one call, released on every path
struct Call {
    hipStream_t s = nullptr;
    void* bufs[8] = {};
    int nb = 0;
    hipError_t err = hipSuccess;
    Call() { err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    ~Call()
    {
        if (s) (void)hipStreamSynchronize(s);
        for (int i = 0; i < nb; ++i) (void)hipFree(bufs[i]);
        if (s) (void)hipStreamDestroy(s);
    }
    template <typename T> T* alloc(size_t n)
    {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 1);
        if (err == hipSuccess) bufs[nb++] = p;
        return (T*)p;
    }
    template <typename T> T* upload(const T* h, size_t n)
    {
        if (!h) return nullptr;
        T* d = alloc<T>(n);
        if (err == hipSuccess) err = hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s);
        return d;
    }
    template <typename T> void download(T* h, const T* d, size_t n)
    {
        if (err == hipSuccess && h) err = hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, s);
    }
    hipError_t finish()
    {
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        return err;
    }
};

constexpr uint64_t kSweepChunk = 1ull << 28;      // evaluations per launch: a few tens of milliseconds

}  // namespace

extern "C" {

// fn: MprobeFn; build: 0 exact, 1 fast, 2 oracle twin.  a, b, c: n floats each (NULL = unused, read as 0);
// out0 (and out1 when not NULL): n result bit patterns (ints for the sign functions, uint32 for to_fixed)
__attribute__((visibility("default"))) hipError_t mprobe_eval(int fn, int build, const float* a, const float* b, const float* c,
                                                              uint32_t* out0, uint32_t* out1, uint64_t n)
{
    if (fn < 0 || fn >= MP_N_FN || build < MP_EXACT || build > MP_ORACLE || !out0) return hipErrorInvalidValue;
    Call k;
    const float* da = k.upload(a, n);
    const float* db = k.upload(b, n);
    const float* dc = k.upload(c, n);
    uint32_t* d0 = k.alloc<uint32_t>(n);
    uint32_t* d1 = out1 ? k.alloc<uint32_t>(n) : nullptr;
    if (k.err != hipSuccess) return k.err;
    if (build == MP_EXACT) k.err = mirt::exact_build::probe_launch_eval(fn, da, db, dc, d0, d1, n, k.s);
    else if (build == MP_FAST) k.err = mirt::fast_build::probe_launch_eval(fn, da, db, dc, d0, d1, n, k.s);
    else {
        hipLaunchKernelGGL(oracle_eval_kernel, dim3(mirt::exact_build::probe_blocks(n)), dim3(256), 0, k.s, fn, da, db, dc, d0, d1, n);
        k.err = hipGetLastError();
    }
    k.download(out0, d0, n);
    k.download(out1, d1, n);
    return k.finish();
}

// product (exact build) vs oracle twin over the patterns [lo, lo + count) (count <= 2^32), for every param where the function
// takes one.  out[3] = {mismatches, smallest mismatching pattern (or index; UINT64_MAX if none), evaluations}
__attribute__((visibility("default"))) hipError_t mprobe_sweep(int fn, uint64_t lo, uint64_t count, const float* params, uint32_t nparams,
                                                               unsigned long long* out)
{
    const bool per_param = fn == MP_SW_ATAN2_Y || fn == MP_SW_ATAN2_X || fn == MP_POW_POS || fn == MP_POW_UNIT;
    const bool known = (fn >= 0 && fn < MP_N_FN) || (fn >= MP_SW_ATAN2_Y && fn <= MP_SW_SIN_PRODUCT);
    if (!known || !out || count > (1ull << 32) || ((per_param || fn == MP_SW_POW_PAIRS) && (!params || !nparams))) return hipErrorInvalidValue;
    Call k;
    const float* dp = k.upload(params, nparams);
    unsigned long long* acc = k.alloc<unsigned long long>(5);
    const unsigned long long init[5] = { 0ull, 0ull, ~0ull, 0ull, 0ull };
    if (k.err == hipSuccess) k.err = hipMemcpyAsync(acc, init, sizeof(init), hipMemcpyHostToDevice, k.s);
    const uint64_t chunk = per_param ? (kSweepChunk / nparams > 0 ? kSweepChunk / nparams : 1) : kSweepChunk;
    for (uint64_t off = 0; off < count && k.err == hipSuccess; off += chunk) {
        const uint64_t c = (count - off < chunk) ? count - off : chunk;
        hipLaunchKernelGGL(sweep_kernel, dim3(mirt::exact_build::probe_blocks(c)), dim3(256), 0, k.s, fn, lo + off, c, dp, nparams, acc);
        k.err = hipGetLastError();
        if (k.err == hipSuccess) k.err = hipStreamSynchronize(k.s);      // one launch in flight: each stays well under a second
    }
    unsigned long long r[5] = {};
    k.download(r, acc, 5);
    if (k.finish() != hipSuccess) return k.err;
    out[0] = r[0];
    out[1] = r[2];
    out[2] = r[3];
    return hipSuccess;
}

// resolve_channel of the exact (0) or fast (1) build, or om_resolve_channel on the device (2), for n sums
__attribute__((visibility("default"))) hipError_t mprobe_resolve(const uint64_t* sums, uint64_t n, uint32_t n_samples, uint32_t flags,
                                                                 int build, uint8_t* out_codes)
{
    if (!sums || !out_codes || n_samples == 0 || build < MP_EXACT || build > MP_ORACLE) return hipErrorInvalidValue;
    Call k;
    const unsigned long long* ds = k.upload((const unsigned long long*)sums, n);
    uint8_t* dc = k.alloc<uint8_t>(n);
    if (k.err != hipSuccess) return k.err;
    if (build == MP_EXACT) k.err = mirt::exact_build::probe_launch_resolve(ds, dc, n, n_samples, flags, k.s);
    else if (build == MP_FAST) k.err = mirt::fast_build::probe_launch_resolve(ds, dc, n, n_samples, flags, k.s);
    else {
        hipLaunchKernelGGL(oracle_resolve_kernel, dim3(mirt::exact_build::probe_blocks(n)), dim3(256), 0, k.s, ds, dc, n, n_samples, flags);
        k.err = hipGetLastError();
    }
    k.download(out_codes, dc, n);
    return k.finish();
}

// the exact resolve vs om_resolve_channel over the sums [sum_lo, sum_lo + count).
// out[5] = {mismatches, monotonicity violations, smallest mismatching sum (UINT64_MAX if none), sums evaluated, largest drop}.
// The oracle's curve itself is not monotone everywhere: uncharted2's f32 quotient minus a constant can step down by one code
// (tests/test_oracle_resolve.py bounds where), so a violation is only an error where the oracle has none.
__attribute__((visibility("default"))) hipError_t mprobe_resolve_sweep(uint32_t n_samples, uint32_t flags, uint64_t sum_lo, uint64_t count,
                                                                       unsigned long long* out)
{
    if (!out || n_samples == 0 || sum_lo + count < sum_lo) return hipErrorInvalidValue;
    Call k;
    unsigned long long* acc = k.alloc<unsigned long long>(5);
    const unsigned long long init[5] = { 0ull, 0ull, ~0ull, 0ull, 0ull };
    if (k.err == hipSuccess) k.err = hipMemcpyAsync(acc, init, sizeof(init), hipMemcpyHostToDevice, k.s);
    constexpr uint64_t kChunk = 1ull << 27;            // sums per launch (two resolves each, with f64 divisions)
    for (uint64_t off = 0; off < count && k.err == hipSuccess; off += kChunk) {
        const uint64_t c = (count - off < kChunk) ? count - off : kChunk;
        const uint64_t runs = (c + 63) / 64;
        hipLaunchKernelGGL(resolve_sweep_kernel, dim3(mirt::exact_build::probe_blocks(runs)), dim3(256), 0, k.s, n_samples, flags,
                           sum_lo, sum_lo + off, c, acc);
        k.err = hipGetLastError();
        if (k.err == hipSuccess) k.err = hipStreamSynchronize(k.s);
    }
    unsigned long long r[5] = {};
    k.download(r, acc, 5);
    if (k.finish() != hipSuccess) return k.err;
    for (int i = 0; i < 5; ++i) out[i] = r[i];
    return hipSuccess;
}

}  // extern "C"
#endif  // !MIRT_FAST_MATH
