// eph_internal.h -- shared declarations of libephemeris_amd (host C++ + HIP kernels for gfx950).
//
// Device data layout (all f64, resident in HBM for the life of a handle):
//   P[2]      : packed bodies {x, y, z, mu} (32 B each, one 2x dwordx4 load per body) -- what the pair kernel
//               streams; ping-pong so a launch can publish the next positions while its peers still read
//               the current ones.
//   Y, A      : history rings [L][3][npad] (level, component, body): positions and accelerations of the last
//               L = ORDER integrator levels (12 for QuinlanTremaine12). Slot `cur` = newest level,
//               (cur + j) % L = j levels back.
//   V         : [3][npad] current velocity.  ASR: [3][npad] SRKN stage acceleration (FSAL carry).
//   samples   : per-body append log of sampled positions (AoS xyz) for the solout windows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>

#include "../../include/ephemeris_amd.h"

namespace eph {

constexpr int kMaxOrder = 16;   // ELM2 orders: 12 (QT12), 13 (Stormer13)
constexpr int kTile = 64;       // one wave64 = one tile of source bodies
constexpr int kRow = 66;        // LDS row stride in doubles of the contribution tile (16-B aligned, conflict-free)
constexpr int kDiv = 8;         // ephemeris/src/trajectory.rs:335  (DIV)
constexpr int kSmallN = 64;     // persistent single-workgroup path handles n <= one tile

struct Body4 { double x, y, z, mu; };
static_assert(sizeof(Body4) == 32, "Body4 must be 32 bytes");

// thread-local HIP error text
void set_last_error(const char *what, hipError_t e);
void set_last_error_text(const std::string &s);
int check_device();  // EPH_OK or EPH_ERR_NO_DEVICE

#define EPH_HIP(call)                                              \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) {                                    \
            ::eph::set_last_error(#call, e_);                      \
            return EPH_ERR_HIP;                                    \
        }                                                          \
    } while (0)

// Launches `kernel` (in parentheses when its template arguments hold a comma) on stream `s`; a launch that fails records `name` as
// the last error and makes the caller return EPH_ERR_HIP. (force_common.h keeps its own launched(): workloads.py hashes that file.)
#define EPH_LAUNCH(name, kernel, grid, block, s, ...)                  \
    do {                                                               \
        hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__);     \
        const hipError_t e_ = hipGetLastError();                       \
        if (e_ != hipSuccess) {                                        \
            ::eph::set_last_error(name, e_);                           \
            return EPH_ERR_HIP;                                        \
        }                                                              \
    } while (0)

// No exception crosses the extern "C" boundary: an entry point's body sits between these two.
#define EPH_GUARD_BEGIN try {
#define EPH_GUARD_END                                                  \
    }                                                                  \
    catch (const std::bad_alloc &) {                                   \
        return EPH_ERR_OUT_OF_MEMORY;                                  \
    }                                                                  \
    catch (...) {                                                      \
        ::eph::set_last_error_text("unexpected C++ exception");        \
        return EPH_ERR_HIP;                                            \
    }

// ---- coefficient tables -> the f64 values the reference multiplies with (coeffs.cpp) ------------
struct SrknCoeffs { int stages = 0; bool fsal = false; double A[32], B[32]; };
struct Elm2Coeffs {
    int order = 0;
    double wa[kMaxOrder], wb[kMaxOrder], cw[kMaxOrder];
    double inv_beta_d = 0, inv_cowell_d = 0;
};
struct ErkCoeffs {             // ERK + embedded pair; A[s][j] for j < s   (integration/src/runge_kutta/explicit.rs:14-38)
    int stages = 0, order = 0, order_embedded = 0;
    int fsal = 0, has_embedded = 0;
    double A[16][16], B[16], C[16], E[16];
    // nystrom = 1: ERKNG pair (runge_kutta/nystrom/explicit_generalized.rs:14-41), at most 8 stages:
    // A = AP, A2 = AV, B = BP, B2 = BV, E = EP, E2 = EV. nystrom = 2: ERKN (nystrom/explicit.rs), the same with A2 = 0
    int nystrom = 0;
    double A2[8][8], B2[8], E2[8];
};
bool find_erk(const char *name, ErkCoeffs *out);
bool find_srkn(const char *name, SrknCoeffs *out);
bool find_elm2(const char *name, Elm2Coeffs *out);

// ---- kernel argument blocks ---------------------------------------------------------------------
struct SampleArgs {            // solout sampling schedule for one batch (device arrays, may be null)
    const uint32_t *period;    // m_b: steps between samples (0 = never)
    const uint32_t *phase;     // r_b: steps since the last sample at batch start
    const uint64_t *offset;    // first free slot of body b in `log` (in samples)
    double *log;               // AoS xyz
};

struct LmArgs {                // fused linear-multistep step (step_wg.hip, step_wave.hip, step_small.hip: k_lm_step_wg / k_lm_step / k_lm_small / k_lm_persistent)
    int n, npad, L, cur;       // cur = ring slot of the level whose acceleration is evaluated
    int lo, hi;                // target bodies [lo, hi) of this launch (0, n unless the system is sharded over ranks)
    const Body4 *pos_cur;      // packed positions of that level
    Body4 *pos_next;           // packed positions of the next level (written when do_predict)
    double *Y, *A, *V;
    double wa[kMaxOrder], wb[kMaxOrder], cw[kMaxOrder];
    double h, hh, hc;          // h, h*h*(1/BETA_D), h*(1/COWELL_D)
    int do_predict;
    uint32_t step;             // 1-based index of this step inside the batch (for sampling)
    int kind;                  // force kernel: 0 auto, 1 wave, 2 workgroup
    int wg_flags;              // workgroup kernel tuning bits (tuning builds: EPH_DEBUG_SMALL, step_small.hip)
    SampleArgs samp;
};

// ---- launchers -------------------------------------------------------------------------------------------------------------------
// The kernels that contain the point-mass term exist once per evaluation order of that term (pair_term.h, pair_ns.h): `pv` (0..6)
// says whose. A handle fixes it at creation (eph_set_pair_variant / EPH_PAIR_VARIANT); dispatch.cpp chooses the kernel form
// (wave / workgroup / single workgroup, bodies per wave or workgroup) and routes to that order's table.
constexpr int kPairVariants = 7;
#define EPH_PAIR_ORDERS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)      // the orders, listed once: the declarations and tables per order
#define EPH_PAIR_ORDER_COUNT(k) +1
static_assert(0 EPH_PAIR_ORDERS(EPH_PAIR_ORDER_COUNT) == kPairVariants, "EPH_PAIR_ORDERS lists every evaluation order once");
#undef EPH_PAIR_ORDER_COUNT
// slot k of a per-order table array holds order k's table (PairKernels below; the hooks' PairDebugKernels, eph_debug.h)
template <class Table>
bool slots_hold_their_orders(const Table *const (&t)[kPairVariants]) {
    for (int k = 0; k < kPairVariants; ++k)
        if (t[k]->variant != k) return false;
    return true;
}
// test hook (eph_debug_wg_cycles of a product build): the kernel launches NBodyIntegration::advance / advance_many have queued on THIS
// thread -- start-up, per-stage, sample and steady launches alike, a gang's shared launch once; read-backs, clones and fits not
void count_launches(uint64_t n);
uint64_t launches_counted();
int default_pair_variant();                 // what new handles take: eph_set_pair_variant, else EPH_PAIR_VARIANT, else 0
int set_default_pair_variant(int pv);       // EPH_ERR_BAD_ARGUMENT outside 0..6
// a[b] = acc_init[b] (or 0) + sum over the other bodies in the reference order; SoA [3][npad] output
// kind: 0 = auto by the number of targets, 1 = one wave per block (wave_force), 2 = workgroup-specialised (wg_force)
// lo, hi: target bodies [lo, hi) (hi < 0: n); lo must be a multiple of 16
// kd (optional): the SRKN stage update fused behind the evaluation, per (body, component) of the launch's targets:
//   v += a * hb ; y += v * ha ; pos_out = y      (symplectic.rs:90-97) -- one launch per stage instead of two
struct KickDrift { double *v, *y; double hb, ha; Body4 *pos_out; };
int launch_accel(int pv, hipStream_t s, int n, int npad, const Body4 *pos, const double *acc_init, double *acc_out,
                 int kind = 0, int lo = 0, int hi = -1, const KickDrift *kd = nullptr);
int launch_lm_step(int pv, hipStream_t s, const LmArgs &a);                 // one fused step, all CUs
int launch_lm_persistent(int pv, hipStream_t s, const LmArgs &a, int64_t nsteps);
// `count` single-workgroup systems (n <= kGangMaxN each, same L), one workgroup each, argv in device memory
constexpr int kGangMaxN = 32;
int launch_lm_small_many(int pv, hipStream_t s, const LmArgs *argv_dev, int count, int L, int64_t nsteps);
// a `<Double>` handle's single-workgroup steps (LmDoubleArgs: double_state.h): n <= kGangMaxN bodies, nsteps per launch
struct LmDoubleArgs;
int launch_lm_double_small(int pv, hipStream_t s, const LmDoubleArgs &d, int64_t nsteps);
// a symplectic (SRKN) handle's single-workgroup steps (step_srkn_small.hip): n <= kGangMaxN bodies, nsteps steps of `stages` stages
// per launch. Stage s: the force at the stage positions (skipped for an FSAL table's first stage once a step has been taken), then
// v += a * hb[s]; y += v * ha[s] on the plain state or on Double (YE / VE: the error parts, `<Double>` handles only).
struct SrknSmallArgs {
    int n, npad;
    int stages, fsal;
    uint32_t starter_i;        // steps the handle has taken on entry: an FSAL table evaluates its first stage at step 0 only
    Body4 *pos[2];             // both packed buffers: pos[0] holds the positions on entry, both hold the newest on exit
    double *Y, *V, *ASR;       // ring slot 0, velocity, the last evaluated acceleration (the FSAL carry across launches)
    double *YE, *VE;
    double hb[32], ha[32];     // h * B[s], h * A[s]: the bound of SrknCoeffs
    SampleArgs samp;           // plain kernel only
};
int launch_srkn_small(int pv, hipStream_t s, const SrknSmallArgs &a, int64_t nsteps);
int launch_srkn_double_small(int pv, hipStream_t s, const SrknSmallArgs &a, int64_t nsteps);
// The gang form of the two (k_srkn_small_many): one workgroup per argument block of a device array, `count` of them. Every block
// carries its own system, table, step and step count -- each member of an advance_many call stops at its own bound, so the count
// cannot be a launch parameter as it is for k_lm_small's gang. One launch holds one state type (plain, or `<Double>`: YE / VE set
// in every block) and one evaluation order.
struct SrknGangArgs {
    SrknSmallArgs s;
    long long nsteps;          // >= 1
};
int launch_srkn_small_many(int pv, hipStream_t s, const SrknGangArgs *argv_dev, int count);
int launch_srkn_double_small_many(int pv, hipStream_t s, const SrknGangArgs *argv_dev, int count);
// a linear multistep handle's start-up in the same frame (k_lm_startup_small, step_srkn_small.hip): `m` macro steps of `substeps`
// steps of the substepper's table `s` per launch, each closed by the force at the new front. s.Y / s.YE are the RING bases, s.starter_i
// counts the substepper's steps (0: the force at the initial positions is evaluated first). The gang form runs one workgroup per
// argument block of a device array (plain state only); every block carries its own system, ring position and m.
struct LmStartupArgs {
    SrknSmallArgs s;
    double *A;                 // acceleration ring [L][3][npad]
    int L, cur;                // ring length; slot of the newest level on entry
    int m, substeps;
};
int launch_lm_startup_small(int pv, hipStream_t s, const LmStartupArgs &a, bool compensated);
int launch_lm_startup_small_many(int pv, hipStream_t s, const LmStartupArgs *argv_dev, int count);
// opt-in fast path: slice-parallel partial sums combined in slice order (NOT the reference's summation order)
int fast_slices(int npad, bool approx = false);                     // S (the rsq form takes twice the waves)
#ifndef EPH_F32_GROUP
#define EPH_F32_GROUP 32
#endif
constexpr int kF32Group = EPH_F32_GROUP;         // EPH_PATH_F32_PAIRS: sources per conversion to f64 (slices are multiples of it)
int fast_unroll();                               // sources per trip of the IEEE form's loop (EPH_FAST_UNROLL: 4, or 8)
int fast_slice_len(int npad, int S, int unroll, bool approx, bool f32);     // sources per slice: npad / S rounded up to the loop's trip
// posf: EPH_PATH_F32_PAIRS scratch, 4 floats per padded body. f32_stage 0: the whole step; 1: only the binary32 copy of rows
// [conv_lo, conv_lo + conv_cnt) (conv_cnt < 0: all); 2: the step on a copy that is complete already (a sharded handle gathers between)
size_t fast_partial_doubles(int npad);           // scratch of the fast paths incl. the arrival tickets behind the partial sums
size_t fast_ticket_offset_doubles(int npad);
int launch_lm_step_fast(int pv, hipStream_t s, const LmArgs &a, double *partial, bool approx, float *posf = nullptr, int f32_stage = 0,
                        int conv_lo = 0, int conv_cnt = -1);
// the massless sweep (craft_sweep.hip); CraftArgs: craft_device.h
struct CraftArgs;
struct CraftLaunch { bool wave_form, queue, occ2; long long resident_waves; };
int launch_craft(int pv, hipStream_t s, const CraftArgs &a, const CraftLaunch &how);
struct PairKernels {                        // one evaluation order's launchers (pair_launchers.h), filled in pair_table.hip
    int (*accel_wave)(hipStream_t, int, int, int, const Body4 *, const double *, double *, int, int, const KickDrift &);
    int (*accel_wg)(hipStream_t, int, int, int, const Body4 *, const double *, double *, int, int, const KickDrift &);
    int (*lm_step_wave)(hipStream_t, int, const LmArgs &);
    int (*lm_step_wg)(hipStream_t, int, const LmArgs &);
    int (*lm_persistent)(hipStream_t, const LmArgs &, int64_t);
    int (*lm_small)(hipStream_t, const LmArgs &, int64_t);
    int (*lm_small_many)(hipStream_t, const LmArgs *, int, int, int64_t);
    int (*lm_double_small)(hipStream_t, const LmDoubleArgs &, int64_t);
    int (*srkn_small)(hipStream_t, const SrknSmallArgs &, int64_t);
    int (*srkn_double_small)(hipStream_t, const SrknSmallArgs &, int64_t);
    int (*srkn_small_many)(hipStream_t, const SrknGangArgs *, int);
    int (*srkn_double_small_many)(hipStream_t, const SrknGangArgs *, int);
    int (*lm_startup_small)(hipStream_t, const LmStartupArgs &, bool);
    int (*lm_startup_small_many)(hipStream_t, const LmStartupArgs *, int);
    int (*lm_step_fast)(hipStream_t, const LmArgs &, double *, int, int, bool, float *, int, int, int, unsigned *);
    int (*craft_launch)(hipStream_t, const CraftArgs &, const CraftLaunch &);
    int variant;                            // the order these launchers were compiled for: dispatch.cpp holds slot k to order k
};
// ---- launchers of the kernels without a point-mass term (solout.hip) --------------------------------------------------------------
int launch_pack(hipStream_t s, int n, int npad, const double *Yslot, const double *mu, Body4 *pos);
int launch_copy3(hipStream_t s, int n, int npad, const double *src, double *dst);
// SRKN stage update: v += a*hb ; y += v*ha ; also publishes packed positions   (symplectic.rs:90-97)
int launch_kick_drift(hipStream_t s, int n, int npad, const double *a, double *v, double *y, double hb, double ha,
                      const double *mu, Body4 *pos_out);
int launch_lm_predict(hipStream_t s, const LmArgs &a);              // y_{m+1} from the ring (no force)
int lm_bodies_per_wave(int n);
int launch_sample(hipStream_t s, int n, int npad, const double *Yslot, const SampleArgs &sa, uint32_t step);
// carry: samples [src[b], src[b]+cnt[b]) of body b's region move to its front (src[b] == 0: nothing to do)
int launch_carry(hipStream_t s, int n, const uint64_t *region, const uint32_t *src, const uint32_t *cnt, double *log);
// AoS <-> SoA staging
int launch_aos_to_soa(hipStream_t s, int n, int npad, const double *aos, double *soa);
int launch_soa_to_aos(hipStream_t s, int n, int npad, const double *soa, double *aos);
// LeastSquaresFit over windows of 9 samples; window w of the launch reads log[(first[w]) .. +8]
int launch_lsq_fit(hipStream_t s, int64_t nwin, const uint64_t *first_sample, const uint8_t *degree, int backward,
                   const double *log, double *coeffs, int32_t *ncoef);
// records of kDiv*3 + 1 doubles per window (coefficients, then ncoef) for the sharded propagator's all-gather
int launch_pack_records(hipStream_t s, int64_t nwin, const double *coeffs, const int32_t *ncoef, double *rec);
int launch_spline_eval(hipStream_t s, int64_t m, const double *at, double start, double interval, int64_t npoly,
                       const double *coeffs, const int32_t *ncoef, double *pos, double *vel, uint8_t *inside);

}  // namespace eph
