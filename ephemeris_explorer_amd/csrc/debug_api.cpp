// debug_api.cpp -- the extern "C" entry points of the test and tuning hooks (csrc/eph_debug.h). Linked into the test-hooks library
// and into tuning builds only: the product library libephemeris_amd.so exports the drop-in boundary and nothing else.
#include <new>

#include "eph_debug.h"
#include "host.h"

using namespace eph;

// the per-order halves of the hooks (pair_debug.hip) and, for eph_debug_table_variants, the product's table (pair_table.hip)
namespace eph {
#define EPH_DECLARE_TABLES(k) namespace pv##k { const PairKernels *pair_table(); const PairDebugKernels *pair_debug_table(); }
EPH_PAIR_ORDERS(EPH_DECLARE_TABLES)
#undef EPH_DECLARE_TABLES
}
// order pv's hooks, as dispatch.cpp's table(pv) for the product's launchers: none for an order that does not exist, or when a slot
// holds another order's table
static const PairDebugKernels *debug_table(int pv) {
#define EPH_TABLE_SLOT(k) pv##k::pair_debug_table(),
    static const PairDebugKernels *const t[kPairVariants] = {EPH_PAIR_ORDERS(EPH_TABLE_SLOT)};
#undef EPH_TABLE_SLOT
    static const bool sound = slots_hold_their_orders(t);
    return sound && pv >= 0 && pv < kPairVariants ? t[pv] : nullptr;
}

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_debug_inv_r3(int64_t n, const double *n2, double *fast, double *ieee) {
    EPH_GUARD_BEGIN
    if (n < 0 || (n > 0 && (!n2 || !fast || !ieee))) return EPH_ERR_BAD_ARGUMENT;
    int st = check_device();
    if (st) return st;
    const PairDebugKernels *t = debug_table(default_pair_variant());
    if (!t) return EPH_ERR_BAD_ARGUMENT;
    if (n == 0) return EPH_OK;
    DevBuf<double> a, b, c;
    if ((st = a.alloc(n)) || (st = b.alloc(n)) || (st = c.alloc(n))) return st;
    EPH_HIP(hipMemcpy(a.p, n2, sizeof(double) * n, hipMemcpyHostToDevice));
    if ((st = t->debug_inv_r3(nullptr, n, a.p, b.p, c.p))) return st;
    EPH_HIP(hipMemcpy(fast, b.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    EPH_HIP(hipMemcpy(ieee, c.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return EPH_OK;
    EPH_GUARD_END
}

// a / (x * sqrt(x)) through the division forms' seeded reciprocal + Markstein step, and through the compiler's IEEE expansions
int32_t eph_debug_quot(int64_t n, const double *x, const double *a, double *fast, double *ieee) {
    EPH_GUARD_BEGIN
    if (n < 0 || (n > 0 && (!x || !a || !fast || !ieee))) return EPH_ERR_BAD_ARGUMENT;
    int st = check_device();
    if (st) return st;
    const PairDebugKernels *t = debug_table(default_pair_variant());
    if (!t) return EPH_ERR_BAD_ARGUMENT;
    if (n == 0) return EPH_OK;
    DevBuf<double> dx, da, b, c;
    if ((st = dx.alloc(n)) || (st = da.alloc(n)) || (st = b.alloc(n)) || (st = c.alloc(n))) return st;
    EPH_HIP(hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
    EPH_HIP(hipMemcpy(da.p, a, sizeof(double) * n, hipMemcpyHostToDevice));
    if ((st = t->debug_quot(nullptr, n, dx.p, da.p, b.p, c.p))) return st;
    EPH_HIP(hipMemcpy(fast, b.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    EPH_HIP(hipMemcpy(ieee, c.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_debug_inv_r3_sweep(uint64_t seed, int64_t n, uint64_t *mismatches, uint64_t *example_bits) {
    EPH_GUARD_BEGIN
    if (n < 0 || !mismatches || !example_bits) return EPH_ERR_BAD_ARGUMENT;
    int st = check_device();
    if (st) return st;
    const PairDebugKernels *t = debug_table(default_pair_variant());
    if (!t) return EPH_ERR_BAD_ARGUMENT;
    DevBuf<unsigned long long> out;
    if ((st = out.alloc(2))) return st;
    EPH_HIP(hipMemset(out.p, 0, 2 * sizeof(unsigned long long)));
    if ((st = t->debug_inv_r3_sweep(nullptr, seed, n, out.p))) return st;
    unsigned long long h[2];
    EPH_HIP(hipMemcpy(h, out.p, sizeof(h), hipMemcpyDeviceToHost));
    *mismatches = h[0];
    *example_bits = h[1];
    return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_debug_wg_cycles(int64_t *out8) {
    if (!out8) return EPH_ERR_BAD_ARGUMENT;
    const PairDebugKernels *t = debug_table(default_pair_variant());
    if (!t) return EPH_ERR_BAD_ARGUMENT;
    const int st = t->debug_wg_cycles((long long *)out8);
#if !EPH_EXPERIMENTS
    if (!st) out8[0] = (int64_t)launches_counted();        // no tick accounting in these objects: the launch accounting instead
#endif
    return st;
}

int32_t eph_debug_div(int64_t n, const double *a, const double *b, double *fast, double *ieee) { return debug_div_device(n, a, b, fast, ieee); }
int32_t eph_debug_rsq(int64_t n, const double *x, double *rsq, double *h) { return debug_rsq_device(n, x, rsq, h); }
int32_t eph_debug_pow(int64_t n, const double *x, double y, double *out) { return debug_pow_device(n, x, y, out); }
int32_t eph_debug_fail_alloc(int32_t nth) { return debug_fail_alloc(nth); }

// host only: the same two helpers launch_lm_step_fast and lm_step_fast call, so a test never restates the partition policy
int32_t eph_debug_fast_partition(int32_t npad, int32_t path, int32_t *S, int32_t *slice_len) {
    if (npad < 64 || npad % 64 || !S || !slice_len) return EPH_ERR_BAD_ARGUMENT;
    if (path != EPH_PATH_FAST && path != EPH_PATH_FAST_RSQ && path != EPH_PATH_F32_PAIRS) return EPH_ERR_BAD_ARGUMENT;
    const bool approx = path == EPH_PATH_FAST_RSQ, f32 = path == EPH_PATH_F32_PAIRS;
    *S = fast_slices(npad, approx);
    *slice_len = fast_slice_len(npad, *S, fast_unroll(), approx, f32);
    return EPH_OK;
}

// host only: what each slot of the two per-order tables says of itself
int32_t eph_debug_table_variants(int32_t *product, int32_t *debug) {
    if (!product || !debug) return EPH_ERR_BAD_ARGUMENT;
#define EPH_TABLE_SLOT(k) product[k] = pv##k::pair_table()->variant, debug[k] = pv##k::pair_debug_table()->variant;
    EPH_PAIR_ORDERS(EPH_TABLE_SLOT)
#undef EPH_TABLE_SLOT
    return EPH_OK;
}

}  // extern "C"
#pragma GCC visibility pop
