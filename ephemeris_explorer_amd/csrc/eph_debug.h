/* eph_debug.h -- test and tuning hooks. NOT part of the drop-in boundary (include/ephemeris_amd.h): no trait of the reference
 * corresponds to them. Their extern "C" entry points are compiled in debug_api.cpp (device halves: debug_kernels.hip and, once per
 * evaluation order of the point-mass term, pair_debug.hip), which is linked into
 *   - libephemeris_amd_testhooks.so (the product's objects + debug_api.o + debug_kernels.o + pair_debug.pv<k>.o; tests/hooks.py
 *     loads it), and
 *   - tuning builds (scripts/build_exp.sh NAME -DEPH_EXPERIMENTS=1 ...),
 * never into libephemeris_amd.so. */
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook: the hardware's v_rsq_f64(x[i]) and the h ~ 0.5/sqrt(x[i]) left by the square root's coupled refinement
 * step -- the inputs of the error-bound note on inv_r3_seeded (csrc/pair_term.h) */
int32_t eph_debug_rsq(int64_t n, const double *x, double *rsq, double *h);
/* Test hook: the step-size controller's correctly rounded pow(x[i], y) on the device */
int32_t eph_debug_pow(int64_t n, const double *x, double y, double *out);
/* test hook: a[i] / b[i] through the shared-reciprocal division of k_craft_wave and through the compiler's IEEE
 * division */
int32_t eph_debug_div(int64_t n, const double *a, const double *b, double *fast, double *ieee);
/* Test hook: 1/(x*sqrt(x)) for n inputs computed by the kernel's in-range fast sequences (NaN where the range
 * guard would send the tile to the IEEE form) and by the compiler's IEEE sqrt/divide expansions. */
int32_t eph_debug_inv_r3(int64_t n, const double *n2, double *fast, double *ieee);
/* a / (x * sqrt(x)): the division forms' shared-reciprocal quotient (csrc/pair_term.h) beside the compiler's IEEE division */
int32_t eph_debug_quot(int64_t n, const double *x, const double *a, double *fast, double *ieee);
/* Test hook: the same comparison over n operands generated on the device (splitmix64(seed + index): random mantissa,
 * exponent uniform over the guarded range; n is rounded up to a multiple of 2^20). *mismatches = operands whose two
 * results differ in any bit; *example_bits = the IEEE bits of one of them (0 when none). */
int32_t eph_debug_inv_r3_sweep(uint64_t seed, int64_t n, uint64_t *mismatches, uint64_t *example_bits);
/* Tuning hook. A build with -DEPH_EXPERIMENTS=1 (scripts/build_exp.sh) returns the single-workgroup kernel's per-phase tick
 * accounting of its last launch (EPH_DEBUG_SMALL=4). The product's objects have no tick accounting: out8[1..7] are zeros and
 * out8[0] is the launch accounting -- the kernel launches that eph_nbody_advance / eph_nbody_advance_many (and the eph_prop_* calls
 * above them) have queued on THIS thread through this library so far: start-up, per-stage, sample and steady launches alike, a
 * launch shared by a gang once; read-backs, clones and fits not counted. Tests read it before and after a call. (The boundary
 * has no such call, and this header no hook of its own for it: both lists of names are pinned by tests/test_abi.py.) */
int32_t eph_debug_wg_cycles(int64_t *out8);
/* Test hook: the nth device allocation the library makes on THIS thread from now (nth >= 1) returns EPH_ERR_OUT_OF_MEMORY with
 * last-error text "injected allocation failure", before any HIP call, and the countdown disarms itself; 0 disarms it. A host
 * function returns an error code: no device is touched. Returns what was left of the previous countdown (0 = it was disarmed). */
int32_t eph_debug_fail_alloc(int32_t nth);
/* Test hook: the partition of the sources that a steady step of `path` (EPH_PATH_FAST, EPH_PATH_FAST_RSQ or EPH_PATH_F32_PAIRS)
 * uses in THIS process for a system padded to npad bodies -- S slices of slice_len consecutive sources, EPH_FAST_SLICES and
 * EPH_FAST_UNROLL honoured. A host function: no device is touched. */
int32_t eph_debug_fast_partition(int32_t npad, int32_t path, int32_t *S, int32_t *slice_len);
/* Test hook: product[k] / debug[k] (7 ints each, one per evaluation order) = the order that slot k of the product's launcher table
 * (csrc/pair_table.hip) and of the hooks' (csrc/pair_debug.hip) was compiled for: k in every slot. A host function: no device is
 * touched. */
int32_t eph_debug_table_variants(int32_t *product, int32_t *debug);

#ifdef __cplusplus
}
#endif

#ifdef __cplusplus
#include <hip/hip_runtime.h>
namespace eph {                 /* the device halves that live beside their kernels (debug_kernels.hip) */
int debug_div_device(int64_t n, const double *a, const double *b, double *fast, double *ieee);
int debug_rsq_device(int64_t n, const double *x, double *rsq, double *h);
int debug_pow_device(int64_t n, const double *x, double y, double *out);
/* one evaluation order's hook launchers, filled in pair_debug.hip: 1/(x*sqrt(x)) and a/(x*sqrt(x)) through the in-range sequences
 * and through the compiler's IEEE expansions; tuning builds (-DEPH_EXPERIMENTS): the single-workgroup kernel's cycle accounting */
struct PairDebugKernels {
    int (*debug_inv_r3)(hipStream_t, int64_t, const double *, double *, double *);
    int (*debug_inv_r3_sweep)(hipStream_t, uint64_t, int64_t, unsigned long long *);
    int (*debug_quot)(hipStream_t, int64_t, const double *, const double *, double *, double *);
    int (*debug_wg_cycles)(long long *);
    int variant;                /* the order they were compiled for: debug_api.cpp holds slot k to order k */
};
}
#endif
