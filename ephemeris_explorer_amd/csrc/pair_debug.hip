// pair_debug.hip -- test hooks: the kernels that evaluate the pieces of the point-mass term (pair_term.h) on their own, their
// launchers and the table debug_api.cpp routes through. Compiled once per evaluation order of the term (pair_ns.h); like
// debug_api.cpp and debug_kernels.hip, linked into the test-hooks library and the tuning builds only.
#include "pair_ns.h"

#include "eph_debug.h"

namespace eph {
namespace EPH_PV_NS {

__global__ void k_debug_inv_r3(long long n, const double *__restrict__ n2, double *__restrict__ fast,
                               double *__restrict__ ieee) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = n2[i];
    fast[i] = in_range(x) ? inv_r3_inrange(x) : __builtin_nan("");
    ieee[i] = inv_r3_ieee(x);
}

// Sweep of the in-range sequence against the compiler's IEEE expansion over counter-generated operands (splitmix64 of
// seed + index: 52 random mantissa bits, biased exponent uniform over the guarded range [723, 1323)). out[0] = number of
// operands whose two results differ in any bit, out[1] = the bits of one such operand.
__global__ void k_debug_inv_r3_sweep(unsigned long long seed, int per_thread, unsigned long long *out) {
    unsigned long long idx = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * (unsigned long long)per_thread;
    unsigned bad = 0;
    unsigned long long bad_x = 0;
    for (int k = 0; k < per_thread; ++k, ++idx) {
        unsigned long long z = seed + idx * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const unsigned long long expo = 723ull + (z >> 52) % 600ull;
        const unsigned long long bits = (expo << 52) | (z & 0xFFFFFFFFFFFFFull);
        const double x = __longlong_as_double((long long)bits);
        const double f = inv_r3_inrange(x), g = inv_r3_ieee(x);
        if (__double_as_longlong(f) != __double_as_longlong(g)) { ++bad; bad_x = bits; }
    }
    if (bad) {
        atomicAdd(&out[0], (unsigned long long)bad);
        atomicExch(&out[1], bad_x);
    }
}

static int debug_inv_r3(hipStream_t s, int64_t n, const double *n2, double *fast, double *ieee) {
    hipLaunchKernelGGL(k_debug_inv_r3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (long long)n, n2, fast, ieee);
    return launched("k_debug_inv_r3");
}
static int debug_inv_r3_sweep(hipStream_t s, uint64_t seed, int64_t n, unsigned long long *out2) {   // rounds n up to 2^20
    const int per = 4096;
    const int64_t threads = (n + per - 1) / per;
    if (threads <= 0) return EPH_OK;
    hipLaunchKernelGGL(k_debug_inv_r3_sweep, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       (unsigned long long)seed, per, out2);
    return launched("k_debug_inv_r3_sweep");
}
// test hook: a / (x * sqrt(x)) through the seeded reciprocal + Markstein step (pair_term.h) and through the compiler's IEEE
// expansions; x in the division forms' guarded range, a in in_range_div (tests/division_hard_cases.py)
__global__ void k_debug_quot(long long n, const double *__restrict__ x, const double *__restrict__ a, double *__restrict__ fast,
                             double *__restrict__ ieee) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p;
    const double r = inv_r3_seeded(x[i], &p);
    fast[i] = div_refined(a[i], p, r);
    ieee[i] = a[i] / (x[i] * sqrt(x[i]));
}
static int debug_quot(hipStream_t s, int64_t n, const double *x, const double *a, double *fast, double *ieee) {
    hipLaunchKernelGGL(k_debug_quot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (long long)n, x, a, fast, ieee);
    return launched("k_debug_quot");
}

// the table debug_api.cpp routes through (a function-local static, as in pair_table.hip)
const PairDebugKernels *pair_debug_table() {
    static const PairDebugKernels t = {debug_inv_r3, debug_inv_r3_sweep, debug_quot, debug_wg_cycles, kPairVariant};
    return &t;
}

}  // namespace EPH_PV_NS
}  // namespace eph
