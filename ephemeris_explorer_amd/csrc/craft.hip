// craft.hip -- the massless path: a batch of independent spacecraft, one device thread each, propagated with an
// adaptive embedded explicit Runge-Kutta pair against the massive bodies' piecewise-polynomial ephemeris.
//
// Mirrors (paths relative to the reference repository root):
//   SpacecraftPropagator::{new, step, reset_integrator}, SpacecraftModel, Timeline, CubicHermiteSplineSolout
//                                                       ephemeris/src/propagators/spacecraft.rs:58-332,415-695
//   AdaptiveRungeKuttaIntegrator::advance, IController::step, PreviousStep
//                                                       integration/src/runge_kutta/mod.rs:188-285,396-440
//   ERK::{advance, error, undo_step}                    integration/src/runge_kutta/explicit.rs:54-141
//   Bodies::acceleration, GravitationalBody::acceleration_at, TNB, ReferenceFrame, AbsTol
//                                                       ephemeris_explorer/src/dynamics/spacecraft.rs:70-74,218-293,609-641
//   UniformSpline::{position, state_vector}             ephemeris/src/trajectory.rs:459-470,551-617
// The live ephemeris table is ephemeris_table.hip, the SOI / apsis search craft_events.hip, the sweep kernels craft_sweep.hip.
// Same f64 operations in the same order as the CPU path; the one libm call on the path, powf in the step-size
// controller, is evaluated correctly rounded in double-double arithmetic on both sides.
#include <chrono>
#include <cstdio>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <shared_mutex>
#include <vector>

#include "craft_batch.h"

namespace eph {

// eph_craft_batch_reset_knots: the newest knot of every craft becomes knot 0 of an otherwise empty slab (the next
// CubicHermiteSpline piece starts where the drained one ended), a KNOTS_FULL status is cleared, and the event
// search's segment cursor moves with the knots.
__global__ void __launch_bounds__(256) k_craft_reset_knots(long long n, int *nknots, int *status, double *knot_t,
                                                           double *knot_y, int *ev_seg, const int *slot_of) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long col = slot_of ? slot_of[i] : i;
    const int nk = nknots[i];
    if (nk > 1) {
        knot_t[col] = knot_t[(long long)(nk - 1) * n + col];
#pragma unroll
        for (int d = 0; d < 6; ++d) knot_y[(long long)d * n + col] = knot_y[((long long)(nk - 1) * 6 + d) * n + col];
        nknots[i] = 1;
        if (ev_seg && ev_seg[i] >= 0) ev_seg[i] = max(ev_seg[i] - (nk - 1), 0);
    }
    if (status[i] == EPH_KNOTS_FULL) status[i] = EPH_OK;
}

// 16 bytes per lane, consecutive lanes consecutive: between device memory and the pinned, device-mapped staging buffer (mem.cpp), either way
__global__ void __launch_bounds__(256) k_copy16(long long n16, const double2 *__restrict__ src, double2 *__restrict__ dst) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i];
}
// few spacecraft: one wave each (k_craft_wave, k_craft_events<true>); many: one thread each. Measured crossover on
// MI355X, Verner87, 32 bodies: see scripts/bench_craft_small.py and profiles/README.md
bool craft_wave_form(long long n_craft) {
    static const int form = [] {
        const char *e = getenv("EPH_CRAFT_FORM");      // "wave" | "thread" (tuning / tests)
        return !e ? 0 : (e[0] == 'w' ? 1 : 2);
    }();
    return form ? form == 1 : n_craft <= kCraftWaveMax;
}
// Which sweep kernel (craft_sweep.hip holds them, once per evaluation order of the point-mass term). The queue form pays when
// craft need very different numbers of attempts AND there are more craft than the chip holds at once (two waves per SIMD), so that
// a finished lane has something to take; a batch whose craft were dealt to the lanes by orbital time scale (a.perm: every
// thread-per-craft batch by default) has waves of similar craft: the static form. EPH_CRAFT_QUEUE=0|1, EPH_CRAFT_OCC=1|2 override
// (tuning, tests).
static int craft_launch(int pv, hipStream_t s, const CraftArgs &a, bool heterogeneous) {
    CraftLaunch how{};
    how.wave_form = craft_wave_form(a.n_craft);
    if (!how.wave_form) {
        static const long long simds = [] {
            int dev = 0, cus = 256;
            if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            return (long long)std::max(cus, 1) * 4;
        }();
        const long long waves = (a.n_craft + 63) / 64;
        static const int forced_q = [] { const char *e = getenv("EPH_CRAFT_QUEUE"); return !e || !*e ? -1 : (e[0] == '0' ? 0 : 1); }();
        how.queue = forced_q >= 0 ? forced_q == 1 : (heterogeneous && !a.perm && waves > 2 * simds);
        if (how.queue) {
            how.resident_waves = std::min(waves, 2 * simds);
            // the queue starts behind the craft the grid's own lanes begin with
            if (hipMemsetAsync(a.queue, 0, sizeof(unsigned long long), s) != hipSuccess ||
                hipMemsetD32Async((hipDeviceptr_t)a.queue, (int)(how.resident_waves * 64), 1, s) != hipSuccess) {
                set_last_error("craft queue reset", hipGetLastError());
                return EPH_ERR_HIP;
            }
        }
        // more waves of craft than SIMDs (256 CUs x 4): hold the kernel to two waves per SIMD
        static const int forced = [] { const char *e = getenv("EPH_CRAFT_OCC"); return e ? atoi(e) : 0; }();
        how.occ2 = forced ? forced == 2 : waves > simds;
    }
    return launch_craft(pv, s, a, how);
}

}  // namespace eph

using namespace eph;

// Scheduling estimate (never part of a result): do the 64 craft that would share a WAVE need very different numbers of
// steps? The step size of an embedded pair follows the local dynamical time sqrt(d^3 / mu) of the nearest massive body,
// so eight waves scattered over the batch (64 consecutive craft each) get tau_i = min over bodies of
// sqrt(|r_i - r_b(t0_i)|^3 / mu_b) from the host copy of the ephemeris (plain Horner; approximate is fine), and the batch
// counts as heterogeneous when inside any of them the largest and smallest tau differ by more than 4x: a low orbit 860 s,
// a heliocentric cruise 5e6 s. Families in contiguous blocks do NOT count (measured: the static kernel is then the
// faster one, 183 against 213 ms -- the hardware's wave dispatch already is a queue of whole waves); craft_launch uses
// the answer to pick k_craft_queue over the static kernel.
// A work estimate per craft for the deal of craft to lanes: the time scale of its ORBIT about its dominant body (the body with
// the smallest local dynamical time sqrt(d^3 / mu)) -- sqrt(a^3 / mu) with the semi-major axis a from the vis-viva energy of the
// relative state when the orbit is bound, 16 x the local value when it is not (a fly-by leaves the body quickly). The LOCAL time
// alone mixes families exactly where the work is: a transfer orbit at perigee and a departing lunar transfer look like a low
// circular orbit (measured: dealing by it, 452 ms against the queue kernel's 347 on the mixed population).
__global__ void __launch_bounds__(256) k_craft_tau(long long n, int n_bodies, const BodyEntry *__restrict__ bodies,
                                                   const double *__restrict__ coeffs, const double *__restrict__ time,
                                                   const double *__restrict__ y, float *__restrict__ tau) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = time[i], px = y[i], py = y[n + i], pz = y[2 * n + i];
    const double vx = y[3 * n + i], vy = y[4 * n + i], vz = y[5 * n + i];
    double best = INFINITY, orbit = INFINITY;
    for (int b = 0; b < n_bodies; ++b) {
        const BodyEntry be = bodies[b];
        if (!(be.mu > 0.0) || be.npoly <= 0) continue;
        long long idx;
        double tq;
        if (!spline_locate(be, t, idx, tq)) continue;
        const double *c = coeffs + (be.coeff_off + idx) * kDiv * 3;
        double bp[3] = {0.0, 0.0, 0.0}, bd[3] = {0.0, 0.0, 0.0};
        for (int k = kDiv - 1; k >= 0; --k)
            for (int d = 0; d < 3; ++d) {
                bd[d] = bd[d] * tq + bp[d];               // derivative with respect to tau, then / interval
                bp[d] = bp[d] * tq + c[k * 3 + d];
            }
        const double dx = px - bp[0], dy = py - bp[1], dz = pz - bp[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        const double local = sqrt(d2 * sqrt(d2) / be.mu);
        if (local < best) {
            best = local;
            const double ux = vx - bd[0] / be.interval, uy = vy - bd[1] / be.interval, uz = vz - bd[2] / be.interval;
            const double energy = 0.5 * (ux * ux + uy * uy + uz * uz) - be.mu / sqrt(d2);
            if (energy < 0.0) {
                const double sma = -be.mu / (2.0 * energy);
                orbit = sqrt(sma * sma * sma / be.mu);
            } else {
                orbit = 16.0 * local;
            }
        }
    }
    tau[i] = (float)orbit;
}
__global__ void __launch_bounds__(256) k_knot0_to_lanes(long long n, const int *__restrict__ perm, const double *__restrict__ time,
                                                        const double *__restrict__ y, double *__restrict__ knot_t,
                                                        double *__restrict__ knot_y) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const long long i = perm[q];
    knot_t[q] = time[i];
    for (int d = 0; d < 6; ++d) knot_y[(long long)d * n + q] = y[(long long)d * n + i];
}
// rows of a [rows][n] slab from lane order back to craft order (eph_craft_batch_knot_slabs of a sorted batch)
__global__ void __launch_bounds__(256) k_rows_to_craft_order(long long rows, long long n, const int *__restrict__ slot_of,
                                                             const double *__restrict__ src, double *__restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long col = slot_of[i];
    for (long long r = 0; r < rows; ++r) dst[r * n + i] = src[r * n + col];
}
// one 80-byte record per craft from the SoA state arrays (coalesced reads, one record per thread written as ten 8-byte words)
__global__ void __launch_bounds__(256) k_craft_summary(long long n, const double *__restrict__ time, const double *__restrict__ y,
                                                       const double *__restrict__ next_h, const int *__restrict__ status,
                                                       const int *__restrict__ nknots, const unsigned *__restrict__ attempts,
                                                       const unsigned *__restrict__ steps, eph_craft_record *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    eph_craft_record r;
    r.t = time[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) { r.pos[d] = y[d * n + i]; r.vel[d] = y[(3 + d) * n + i]; }
    r.next_h = next_h[i];
    r.status = status[i];
    r.nknots = nknots[i];
    r.attempts = attempts[i];
    r.steps = steps[i];
    out[i] = r;
}
// the ephemeris's table entries in the order Bodies::acceleration visits them (eph_craft_batch_set_body_order), gathered from the LIVE
// table before every sweep: the entries change when the ephemeris grows
__global__ void __launch_bounds__(64) k_permute_bodies(int n, const int *__restrict__ order, const BodyEntry *__restrict__ table,
                                                       BodyEntry *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = table[order[q]];
}
// Which craft a lane integrates is free (craft are independent, every craft's operations are the reference's whoever runs them),
// so every thread-per-craft batch is dealt to the lanes in the order of k_craft_tau's estimate -- a stable radix sort on the host,
// shortest orbit first (most steps first). The lanes of a wave then carry craft of similar step counts: on the mixed population
// 185 against 343 ms with the queue kernel in craft order (profiles/r03_craft_queue.md); on the north star's own sweep (one
// transfer arc +- 100 km) the accepted steps of a craft follow its orbital energy with correlation -0.99, and the deal takes the
// max / mean steps per wave from 1.09 to 1.01 (oracle, 1500 craft). The knot slabs keep LANE columns (coalesced knot writes
// whatever the deal); every reader translates through the inverse. EPH_CRAFT_SORT=0 switches it off (tuning, tests).
// EPH_CRAFT_SORT: 0 = never deal | 1 = heterogeneous batches only (round 3's default) | unset / 2 = every thread-per-craft batch
static int craft_sort_mode() {
    static const int mode = [] { const char *e = getenv("EPH_CRAFT_SORT"); return !e || !*e ? 2 : (e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2)); }();
    return mode;
}
int eph::craft_sort(eph_craft_batch *b, bool knot0_to_lanes) {
    const long long n = b->n;
    const int mode = craft_sort_mode();
    if (craft_wave_form(n) || mode == 0 || (mode == 1 && !b->heterogeneous) || n < 128 || n > 0x7fffffffLL) return EPH_OK;
    // Transfers through the process's pinned staging buffer (mem.cpp), moved by kernels: no pinning and unpinning of three
    // short-lived host vectors per creation.
    const size_t n4 = ((size_t)n + 3) & ~(size_t)3;    // 16-byte granules for k_copy16
    DevBuf<float> tau;
    int st = tau.alloc(n4);
    if (st) return st;
    StreamIdleOnExit idle(b->stream);                  // (declared after tau: a failed allocation below leaves with k_craft_tau done)
    EPH_LAUNCH("k_craft_tau", k_craft_tau, dim3((unsigned)((n + 255) / 256)), dim3(256), b->stream, n, b->eph->n_bodies, b->eph->bodies.p,
               b->eph->coeffs.p, b->time.p, b->y.p, tau.p);
    if ((st = alloc_buffers(b, BatchDims{n, 0, 0, 0, 0, 0}, [](BufGroup g) { return g == BufGroup::deal; }))) return st;   // perm, slot_of: n4 each
    PinnedStage stage(2 * n4 * sizeof(int));
    if (stage.status()) return stage.status();
    const unsigned cgrid = (unsigned)std::min<size_t>((n4 / 4 + 255) / 256, 4096);
    EPH_LAUNCH("k_copy16", k_copy16, dim3(cgrid), dim3(256), b->stream, (long long)(n4 / 4), (const double2 *)tau.p, (double2 *)stage.dev());
    EPH_HIP(hipStreamSynchronize(b->stream));
    const float *h = static_cast<const float *>(stage.host());
    // stable LSD radix sort of the estimates (positive binary32 values order like their bit patterns; anything else goes last)
    std::vector<uint32_t> key((size_t)n);
    for (long long i = 0; i < n; ++i) {
        const float v = h[(size_t)i];
        uint32_t u;
        std::memcpy(&u, &v, sizeof(u));
        key[(size_t)i] = v > 0.0f && std::isfinite(v) ? u : 0xffffffffu;
    }
    std::vector<int> perm((size_t)n), other((size_t)n);
    for (long long i = 0; i < n; ++i) perm[(size_t)i] = (int)i;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<long long> start(65536 + 1, 0);
        const int shift = 16 * pass;
        for (long long q = 0; q < n; ++q) start[((key[(size_t)perm[(size_t)q]] >> shift) & 0xffffu) + 1] += 1;
        for (int d = 0; d < 65536; ++d) start[d + 1] += start[d];
        for (long long q = 0; q < n; ++q) {
            const int c = perm[(size_t)q];
            other[(size_t)start[(key[(size_t)c] >> shift) & 0xffffu]++] = c;
        }
        perm.swap(other);
    }
    std::vector<int> slot((size_t)n);
    for (long long q = 0; q < n; ++q) slot[(size_t)perm[(size_t)q]] = (int)q;
    int *hp = static_cast<int *>(stage.host());
    std::memcpy(hp, perm.data(), sizeof(int) * (size_t)n);
    std::memcpy(hp + n4, slot.data(), sizeof(int) * (size_t)n);
    const int *dp = static_cast<const int *>(stage.dev());
    EPH_LAUNCH("k_copy16", k_copy16, dim3(cgrid), dim3(256), b->stream, (long long)(n4 / 4), (const double2 *)dp, (double2 *)b->perm.p);
    EPH_LAUNCH("k_copy16", k_copy16, dim3(cgrid), dim3(256), b->stream, (long long)(n4 / 4), (const double2 *)(dp + n4), (double2 *)b->slot_of.p);
    b->h_slot = std::move(slot);
    // knot 0 (the initial state, uploaded in craft order) moves to the lanes' columns
    if (knot0_to_lanes)
        EPH_LAUNCH("k_knot0_to_lanes", k_knot0_to_lanes, dim3((unsigned)((n + 255) / 256)), dim3(256), b->stream, n, b->perm.p, b->time.p,
                   b->y.p, b->knot_t.p, b->knot_y.p);
    EPH_HIP(hipStreamSynchronize(b->stream));
    return EPH_OK;
}

static bool craft_time_scales_differ(const eph_ephemeris &e, long long n, const double *t0, const double *pos) {
    if (n < 128 || e.splines.empty()) return false;
    auto tau_of = [&](long long i) {
        double best = INFINITY;
        for (size_t q = 0; q < e.splines.size(); ++q) {
            const UniformSpline &u = e.splines[q];
            const double mu = e.gm[q];
            const long long npoly = (long long)u.polynomials.size();
            if (!(mu > 0.0) || npoly <= 0) continue;
            const double local = t0[i] - u.start;
            if (!(local >= 0.0) || local > u.span()) continue;
            long long idx = (long long)std::ceil(local / u.interval) - 1;
            idx = std::min(std::max<long long>(idx, 0), npoly - 1);
            const double tq = (local - u.interval * (double)idx) / u.interval;
            const Polynomial &p = u.polynomials[(size_t)idx];
            double bp[3] = {0.0, 0.0, 0.0};
            for (int k = std::min(std::max(p.ncoef, 0), kDiv) - 1; k >= 0; --k)
                for (int d = 0; d < 3; ++d) bp[d] = bp[d] * tq + p.c[k][d];
            const double dx = pos[3 * i] - bp[0], dy = pos[3 * i + 1] - bp[1], dz = pos[3 * i + 2] - bp[2];
            const double d2 = dx * dx + dy * dy + dz * dz;
            best = std::min(best, std::sqrt(d2 * std::sqrt(d2) / mu));
        }
        return best;
    };
    const long long waves = n / 64;
    for (int w = 0; w < 8; ++w) {
        const long long first = (long long)(((unsigned long long)w * 0x9E3779B97F4A7C15ull >> 11) % (unsigned long long)waves) * 64;
        double lo = INFINITY, hi = 0.0;
        for (long long i = first; i < first + 64; ++i) {
            const double t = tau_of(i);
            if (!std::isfinite(t)) continue;
            lo = std::min(lo, t);
            hi = std::max(hi, t);
        }
        if (hi > 4.0 * lo) return true;
    }
    return false;
}

// Timeline::new  ephemeris/src/propagators/spacecraft.rs:129-152: stable sort by start, coast segments in the gaps,
// from Epoch::MIN to Epoch::MAX; appended to `segs`
void eph::timeline_new(long long nburns, const double *burn_start, const double *burn_end, const double *burn_acc,
                       const int32_t *burn_ref, std::vector<SegmentDev> &segs) {
    const double EMIN = -1.7976931348623157e308, EMAX = 1.7976931348623157e308;   // Epoch::MIN / MAX
    std::vector<long long> order;
    for (long long q = 0; q < nburns; ++q) order.push_back(q);
    std::stable_sort(order.begin(), order.end(), [&](long long x, long long y) { return burn_start[x] < burn_start[y]; });
    double cursor = EMIN;
    for (long long q : order) {
        if (burn_start[q] > cursor) segs.push_back(SegmentDev{cursor, burn_start[q], 0, 0, 0, 0, -1});
        cursor = burn_end[q];
        segs.push_back(SegmentDev{burn_start[q], burn_end[q], burn_acc[3 * q], burn_acc[3 * q + 1], burn_acc[3 * q + 2],
                                  1, burn_ref[q]});
    }
    if (cursor < EMAX) segs.push_back(SegmentDev{cursor, EMAX, 0, 0, 0, 0, -1});
}

int eph::burn_csr_check(long long n, const int64_t *burn_offset, const double *burn_start, const double *burn_end, const double *burn_acc,
                        const int32_t *burn_ref, int n_bodies, const uint8_t *which, bool from_zero) {
    if (!burn_offset) return EPH_OK;
    if (burn_offset[0] < 0) return EPH_ERR_BAD_ARGUMENT;
    for (long long i = 0; i < n; ++i)
        if (burn_offset[i + 1] < burn_offset[i]) return EPH_ERR_BAD_ARGUMENT;
    if (burn_offset[n] > (from_zero ? 0 : burn_offset[0]) && (!burn_start || !burn_end || !burn_acc || !burn_ref)) return EPH_ERR_BAD_ARGUMENT;
    for (long long i = 0; i < n; ++i)
        for (int64_t q = burn_offset[i]; (!which || which[i]) && q < burn_offset[i + 1]; ++q)
            if (burn_ref[q] < -1 || burn_ref[q] >= n_bodies) return EPH_ERR_BAD_ARGUMENT;
    return EPH_OK;
}
// ERKN integrates y'' = f(t, y) (P::ODE: SecondOrderODE, nystrom/explicit.rs:60): the spacecraft model is one only while no burn is
// expressed in a frame built from the velocity (ReferenceFrame::Relative -> TNB of the relative state,
// dynamics/spacecraft.rs:281-293). The reference cannot even express that combination.
int eph::burn_erkn_check(long long n, const int64_t *burn_offset, const int32_t *burn_ref, const uint8_t *which) {
    for (long long i = 0; burn_offset && i < n; ++i)
        for (int64_t q = burn_offset[i]; (!which || which[i]) && q < burn_offset[i + 1]; ++q)
            if (burn_ref[q] >= 0) {
                set_last_error_text("Tsitouras75Nystrom (ERKN) needs a velocity-independent right-hand side: "
                                    "burns must use the inertial frame");
                return EPH_ERR_UNSUPPORTED;
            }
    return EPH_OK;
}

int eph::craft_batch_shell(const eph_craft_batch &model, long long n, int max_knots, std::unique_ptr<eph_craft_batch> &out) {
    out.reset(new eph_craft_batch());                                 // (a failure below: it leaves with the caller's pointer)
    eph_craft_batch *b = out.get();
    b->pv = model.pv; b->eph = model.eph; b->device = model.device; b->rk = model.rk; b->params = model.params; b->events = model.events;
    b->max_tr = model.max_tr; b->max_ap = model.max_ap; b->retry = model.retry; b->body_order = model.body_order;
    b->heterogeneous = model.heterogeneous; b->n = n; b->max_knots = max_knots;
    EPH_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    EPH_HIP(hipEventCreate(&b->ev0));
    EPH_HIP(hipEventCreate(&b->ev1));
    return EPH_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_create(const eph_ephemeris *e, int64_t n_craft, const double *t0, const double *pos,
                               const double *vel, const char *method, const eph_adaptive_params *params,
                               const int64_t *burn_offset, const double *burn_start, const double *burn_end,
                               const double *burn_acc, const int32_t *burn_ref, int32_t max_knots,
                               eph_craft_batch **out) {
    EPH_GUARD_BEGIN
        if (!e || n_craft < 0 || !method || !params || !out || max_knots < 1 || (n_craft > 0 && (!t0 || !pos || !vel)))
            return EPH_ERR_BAD_ARGUMENT;
        // the burn tables are caller memory: validate before the first dereference
        int st = burn_csr_check(n_craft, burn_offset, burn_start, burn_end, burn_acc, burn_ref, e->n_bodies, nullptr, true);
        if (st || (st = check_device())) return st;
        std::shared_lock<std::shared_mutex> table_lock(e->mu);       // (the deal to the lanes reads the table)
        eph_craft_batch model;                                       // the settings a batch carries, from the arguments
        if (!find_erk(method, &model.rk) || !model.rk.has_embedded) return EPH_ERR_BAD_ARGUMENT;
        if (model.rk.nystrom == 2 && (st = burn_erkn_check(n_craft, burn_offset, burn_ref, nullptr))) return st;
        model.pv = default_pair_variant(); model.eph = e; model.params = *params; model.device = e->device;
        EPH_HIP(hipSetDevice(model.device));
        std::unique_ptr<eph_craft_batch> b;
        if ((st = craft_batch_shell(model, n_craft, max_knots, b))) return st;
        const long long n = n_craft;
        // Timeline::new per craft  spacecraft.rs:129-152
        std::vector<long long> seg_off(n + 1, 0);
        std::vector<SegmentDev> segs;
        std::vector<int> cur(n, 0);
        for (long long i = 0; i < n; ++i) {
            seg_off[i] = (long long)segs.size();
            const long long b0 = burn_offset ? burn_offset[i] : 0, b1 = burn_offset ? burn_offset[i + 1] : 0;
            timeline_new(b1 - b0, burn_start + b0, burn_end + b0, burn_acc + 3 * b0, burn_ref + b0, segs);
            // segment_idx_at(t0): partition_point(seg.end() <= time)
            int idx = 0;
            const long long ns = (long long)segs.size() - seg_off[i];
            while (idx < ns && segs[seg_off[i] + idx].end <= t0[i]) ++idx;
            cur[i] = idx;
        }
        seg_off[n] = (long long)segs.size();
        if ((st = alloc_state(b.get(), n, max_knots, segs.size()))) return st;
        EPH_HIP(hipMemcpy(b->rk_dev.p, &b->rk, sizeof(ErkCoeffs), hipMemcpyHostToDevice));
        if (n > 0) {
            std::vector<double> ysoa(6 * n), hs(n, params->h_init);
            for (long long i = 0; i < n; ++i)
                for (int d = 0; d < 3; ++d) { ysoa[d * n + i] = pos[3 * i + d]; ysoa[(3 + d) * n + i] = vel[3 * i + d]; }
            std::vector<int> ones(n, 1), zeros(n, 0);
            EPH_HIP(hipMemcpy(b->time.p, t0, sizeof(double) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->last_knot.p, t0, sizeof(double) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->t_start.p, t0, sizeof(double) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->y.p, ysoa.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->klast.p, ysoa.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->kfirst.p, ysoa.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice));   // from_problem: k = [state; STAGES]
            EPH_HIP(hipMemcpy(b->next_h.p, hs.data(), sizeof(double) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemset(b->n_attempts.p, 0, sizeof(unsigned) * n));
            EPH_HIP(hipMemset(b->rk_i.p, 0, sizeof(unsigned) * n));
            EPH_HIP(hipMemset(b->steps.p, 0, sizeof(unsigned) * n));
            EPH_HIP(hipMemcpy(b->cur_seg.p, cur.data(), sizeof(int) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->status.p, zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->nknots.p, ones.data(), sizeof(int) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->seg_off.p, seg_off.data(), sizeof(long long) * (n + 1), hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->segs.p, segs.data(), sizeof(SegmentDev) * segs.size(), hipMemcpyHostToDevice));
            // knot 0 = the initial state (CubicHermiteSplineSolout::new_solution)
            EPH_HIP(hipMemcpy(b->knot_t.p, t0, sizeof(double) * n, hipMemcpyHostToDevice));
            EPH_HIP(hipMemcpy(b->knot_y.p, ysoa.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice));
            b->heterogeneous = craft_time_scales_differ(*e, n, t0, pos);
            if ((st = craft_sort(b.get(), true))) return st;
        }
        b->h_seg_off = std::move(seg_off);
        b->h_segs = std::move(segs);
        *out = b.release();
        return EPH_OK;
    EPH_GUARD_END
}

static int32_t craft_run(eph_craft_batch *b, double t_end, unsigned step_limit);
int32_t eph_craft_batch_propagate(eph_craft_batch *b, double t_end) { return craft_run(b, t_end, 0); }
// IncrementalPropagator::step, n times, for every craft  (ephemeris/src/lib.rs:40-47, spacecraft.rs:598-615)
int32_t eph_craft_batch_step_n(eph_craft_batch *b, uint32_t n_steps) {
    if (n_steps == 0) return b ? EPH_OK : EPH_ERR_BAD_ARGUMENT;
    return craft_run(b, 1.7976931348623157e308, n_steps);
}
static int32_t craft_run(eph_craft_batch *b, double t_end, unsigned step_limit) {
    if (!b) return EPH_ERR_BAD_ARGUMENT;
    if (b->n == 0) return EPH_OK;
    EPH_HIP(hipSetDevice(b->device));
    // the reference's RwLock read guard (dynamics/mod.rs:84-85), held for the whole synchronous sweep: the table as it is NOW --
    // every append since the last call is seen, and none lands while the kernels read
    std::shared_lock<std::shared_mutex> table_lock(b->eph->mu);
    StreamIdleOnExit idle(b->stream);      // (destroyed before the lock: an early error return lets no writer in under kernels in flight)
    if (!b->body_order.empty()) {
        EPH_LAUNCH("k_permute_bodies", k_permute_bodies, dim3((unsigned)((b->eph->n_bodies + 63) / 64)), dim3(64), b->stream,
                   b->eph->n_bodies, b->body_order_dev.p, b->eph->bodies.p, b->bodies_ordered.p);
    }
    CraftArgs a{};
    a.n_craft = b->n;
    a.n_bodies = b->eph->n_bodies;
    a.bodies = b->bodies_ordered.p ? b->bodies_ordered.p : b->eph->bodies.p;
    a.bodies_by_index = b->eph->bodies.p;
    a.coeffs = b->eph->coeffs.p; a.ncoef = b->eph->ncoef.p;
    a.time = b->time.p; a.y = b->y.p; a.next_h = b->next_h.p; a.klast = b->klast.p; a.kfirst = b->kfirst.p; a.last_knot_t = b->last_knot.p;
    a.retry = b->retry ? 1 : 0;
    a.n_attempts = b->n_attempts.p; a.rk_i = b->rk_i.p; a.steps = b->steps.p;
    a.cur_seg = b->cur_seg.p; a.status = b->status.p; a.nknots = b->nknots.p;
    a.seg_off = b->seg_off.p; a.segs = b->segs.p;
    a.knot_t = b->knot_t.p; a.knot_y = b->knot_y.p; a.max_knots = b->max_knots;
    a.rk = b->rk;
    a.rkd = b->rk_dev.p;
    a.h_init = b->params.h_init; a.h_max = b->params.h_max; a.tol_pos = b->params.tol_position;
    a.tol_vel = b->params.tol_velocity; a.fac_min = b->params.fac_min; a.fac_max = b->params.fac_max;
    a.fac = b->params.fac; a.n_max = b->params.n_max;
    a.t_end = t_end;
    a.step_limit = step_limit;
    a.queue = b->queue.p;
    a.perm = b->perm.p;
    EPH_HIP(hipEventRecord(b->ev0, b->stream));
    int st = craft_launch(b->pv, b->stream, a, b->heterogeneous);
    if (st) return st;
    b->retry = false;                      // consumed by a sweep that was launched: a failed launch leaves the batch re-armed
    if (b->events && (st = craft_events_search(b, b->stream))) return st;   // the app's SpacecraftSolout on the steps just taken
    EPH_HIP(hipEventRecord(b->ev1, b->stream));
    EPH_HIP(hipEventSynchronize(b->ev1));
    idle.disarm();
    float ms = 0;
    EPH_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    b->kernel_ms += ms;
    return EPH_OK;
}

int32_t eph_craft_batch_status(eph_craft_batch *b, int32_t *status, int32_t *nknots, uint32_t *attempts, uint32_t *steps) {
    if (!b) return EPH_ERR_BAD_ARGUMENT;
    EPH_HIP(hipSetDevice(b->device));
    const size_t n = (size_t)b->n;
    if (n == 0) return EPH_OK;
    if (status) EPH_HIP(hipMemcpy(status, b->status.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (nknots) EPH_HIP(hipMemcpy(nknots, b->nknots.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (attempts) EPH_HIP(hipMemcpy(attempts, b->n_attempts.p, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    if (steps) EPH_HIP(hipMemcpy(steps, b->steps.p, sizeof(unsigned) * n, hipMemcpyDeviceToHost));
    return EPH_OK;
}

int32_t eph_craft_batch_state(eph_craft_batch *b, double *t, double *pos, double *vel, double *next_h) {
    if (!b) return EPH_ERR_BAD_ARGUMENT;
    EPH_HIP(hipSetDevice(b->device));
    const long long n = b->n;
    if (n == 0) return EPH_OK;
    if (t) EPH_HIP(hipMemcpy(t, b->time.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (next_h) EPH_HIP(hipMemcpy(next_h, b->next_h.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (pos || vel) {
        std::vector<double> y(6 * n);
        EPH_HIP(hipMemcpy(y.data(), b->y.p, sizeof(double) * 6 * n, hipMemcpyDeviceToHost));
        for (long long i = 0; i < n; ++i)
            for (int d = 0; d < 3; ++d) {
                if (pos) pos[3 * i + d] = y[d * n + i];
                if (vel) vel[3 * i + d] = y[(3 + d) * n + i];
            }
    }
    return EPH_OK;
}

// One 80-byte record per craft packed on the device, one copy into the caller's memory.
// Round 3's "2-38 ms in summary()" (profiles/r04_sweep_evidence.md): the FIRST read-back after a burst of batch creations starts
// 15-40 ms late ON THE DEVICE -- rocprofv3 shows the pack kernel's launch issued 1 ms after the sweep kernel ended and the kernel
// starting 20-30 ms later with the queue idle and no host thread busy. It is a one-off per burst of creations (every later
// read-back takes 0.4 ms for 21 MB), it is there with the copy engine out of the picture (records stored by a kernel into pinned
// host memory: same delay), without hipFree, without scratch, on a shared stream; a read-back issued after the LAST creation
// absorbs it, one at the end of each creation does not. bench.py therefore reads every batch back once before its timed region.
// EPH_TRACE_SUMMARY=1 prints the host timers of the phases.
int32_t eph_craft_batch_summary(eph_craft_batch *b, eph_craft_record *out) {
    if (!b || (b->n > 0 && !out)) return EPH_ERR_BAD_ARGUMENT;
    if (b->n == 0) return EPH_OK;
    EPH_HIP(hipSetDevice(b->device));
    static const int trace = [] { const char *e = getenv("EPH_TRACE_SUMMARY"); return e ? atoi(e) : 0; }();
    const auto tick = [] { return std::chrono::steady_clock::now(); };
    const auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point c) {
        return std::chrono::duration<double, std::micro>(c - a).count(); };
    const auto t0 = tick();
    int st;
    if ((st = b->summary.reserve((size_t)b->n))) return st;
    EPH_LAUNCH("k_craft_summary", k_craft_summary, dim3((unsigned)((b->n + 255) / 256)), dim3(256), b->stream, b->n, b->time.p, b->y.p,
               b->next_h.p, b->status.p, b->nknots.p, b->n_attempts.p, b->steps.p, b->summary.p);
    const auto t1 = tick();
    EPH_HIP(hipMemcpyAsync(out, b->summary.p, sizeof(eph_craft_record) * (size_t)b->n, hipMemcpyDeviceToHost, b->stream));
    const auto t2 = tick();
    EPH_HIP(hipStreamSynchronize(b->stream));
    if (trace) fprintf(stderr, "summary: pack launch %.0f memcpyAsync %.0f sync %.0f us\n", us(t0, t1), us(t1, t2), us(t2, tick()));
    return EPH_OK;
}

// The order in which Bodies::acceleration adds the massive bodies' terms (dynamics/spacecraft.rs:222-228 iterates an EntityHashMap:
// unspecified upstream). Table (file) order by default -- the library test's IndexMap; a maintainer who wants the bits of a given
// app run passes that run's iteration order here. Burn reference bodies, SOI radii and event body indices keep the table's numbering.
int32_t eph_craft_batch_set_body_order(eph_craft_batch *b, const int32_t *order) {
    EPH_GUARD_BEGIN
        if (!b) return EPH_ERR_BAD_ARGUMENT;
        EPH_HIP(hipSetDevice(b->device));
        EPH_HIP(hipStreamSynchronize(b->stream));
        if (!order) { b->bodies_ordered.release(); b->body_order_dev.release(); b->body_order.clear(); return EPH_OK; }
        const int n = b->eph->n_bodies;
        std::vector<char> seen((size_t)std::max(n, 1), 0);
        for (int q = 0; q < n; ++q) {
            if (order[q] < 0 || order[q] >= n || seen[(size_t)order[q]]) return EPH_ERR_BAD_ARGUMENT;   // not a permutation
            seen[(size_t)order[q]] = 1;
        }
        // the sweep kernels walk a.bodies front to back: a permuted COPY of the ephemeris's table costs the kernels nothing (an index
        // array read inside the body loop cost the thread-per-craft kernel 5 %: 35.0 against 33.4 ms); craft_run re-gathers it from
        // the live table before every sweep (k_permute_bodies)
        // built aside and swapped in: on any failure the batch keeps the order it had, or none
        int st;
        DevBuf<BodyEntry> ordered;
        DevBuf<int> order_dev;
        if ((st = ordered.alloc((size_t)std::max(n, 1))) || (st = order_dev.alloc((size_t)std::max(n, 1)))) return st;
        std::vector<int32_t> host(order, order + n);
        if (n) EPH_HIP(hipMemcpy(order_dev.p, order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        b->bodies_ordered.swap(ordered);
        b->body_order_dev.swap(order_dev);
        b->body_order.swap(host);
        return EPH_OK;
    EPH_GUARD_END
}
// IncrementalPropagator::step on a propagator whose last step returned Err (ephemeris/src/propagators/spacecraft.rs:598-615): nothing
// in the reference remembers the failure -- the next step() simply runs AdaptiveRungeKuttaIntegrator::advance again from the state the
// failed attempt left (runge_kutta/mod.rs:414-439). A sweep must not do that implicitly (a drain loop would re-attempt the failed craft
// of a batch on every pass, and a failed attempt is not idempotent: see the header), so the batch keeps a StepError sticky until this
// call re-arms it: the NEXT propagate / step_n then steps every craft whatever its last status.
int32_t eph_craft_batch_retry_failed(eph_craft_batch *b) {
    if (!b) return EPH_ERR_BAD_ARGUMENT;
    b->retry = true;
    return EPH_OK;
}

int32_t eph_craft_batch_knots(eph_craft_batch *b, int64_t craft, double *t, double *pos, double *vel) {
    if (!b || craft < 0 || craft >= b->n) return EPH_ERR_BAD_ARGUMENT;
    EPH_HIP(hipSetDevice(b->device));
    int nk = 0;
    EPH_HIP(hipMemcpy(&nk, b->nknots.p + craft, sizeof(int), hipMemcpyDeviceToHost));
    const long long n = b->n;
    const long long col = b->h_slot.empty() ? craft : b->h_slot[(size_t)craft];
    // strided gather: knot k of craft i sits at [k*n + col(i)] (col = i unless the batch was dealt to the lanes by craft_sort)
    if (t) EPH_HIP(hipMemcpy2D(t, sizeof(double), b->knot_t.p + col, sizeof(double) * n, sizeof(double), nk,
                               hipMemcpyDeviceToHost));
    if (pos || vel) {
        std::vector<double> y((size_t)nk * 6);
        EPH_HIP(hipMemcpy2D(y.data(), sizeof(double), b->knot_y.p + col, sizeof(double) * n, sizeof(double),
                            (size_t)nk * 6, hipMemcpyDeviceToHost));
        for (int k = 0; k < nk; ++k)
            for (int d = 0; d < 3; ++d) {
                if (pos) pos[3 * k + d] = y[(size_t)k * 6 + d];
                if (vel) vel[3 * k + d] = y[(size_t)k * 6 + 3 + d];
            }
    }
    return EPH_OK;
}

// Timeline::divergence_time_before  spacecraft.rs:179-213 (common_times: segments zipped while their starts agree,
// stopping after the first pair whose thrust differs; the last such start that is < before)
int32_t eph_timeline_divergence_time(int64_t n_old, const double *old_start, const double *old_end, const double *old_acc,
                                     const int32_t *old_ref, int64_t n_new, const double *new_start,
                                     const double *new_end, const double *new_acc, const int32_t *new_ref,
                                     double before, double *restart_epoch) {
    EPH_GUARD_BEGIN
        if (n_old < 0 || n_new < 0 || !restart_epoch || (n_old > 0 && (!old_start || !old_end || !old_acc || !old_ref)) ||
            (n_new > 0 && (!new_start || !new_end || !new_acc || !new_ref)))
            return EPH_ERR_BAD_ARGUMENT;
        std::vector<SegmentDev> a, b;
        timeline_new(n_new, new_start, new_end, new_acc, new_ref, a);     // self = the new timeline
        timeline_new(n_old, old_start, old_end, old_acc, old_ref, b);
        bool done = false, any = false;
        double last = 0.0;
        for (size_t k = 0; k < a.size() && k < b.size(); ++k) {
            if (done || a[k].start != b[k].start) break;
            const double t = a[k].start;
            // s1.thrust() != s2.thrust(): Option<ConstantThrust { acceleration, frame }>
            const bool same = a[k].is_burn == b[k].is_burn &&
                              (!a[k].is_burn || (a[k].ax == b[k].ax && a[k].ay == b[k].ay && a[k].az == b[k].az &&
                                                 a[k].ref == b[k].ref));
            if (!same) done = true;
            if (!(t < before)) break;                                    // take_while(|&t| t < before)
            last = t;
            any = true;
        }
        if (!any) return EPH_ERR_BAD_ARGUMENT;                           // the reference unwraps (before <= Epoch::MIN)
        *restart_epoch = last;
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_craft_batch_reset_knots(eph_craft_batch *b) {
    if (!b) return EPH_ERR_BAD_ARGUMENT;
    if (b->n == 0) return EPH_OK;
    EPH_HIP(hipSetDevice(b->device));
    EPH_LAUNCH("k_craft_reset_knots", k_craft_reset_knots, dim3((unsigned)((b->n + 255) / 256)), dim3(256), b->stream, b->n,
               b->nknots.p, b->status.p, b->knot_t.p, b->knot_y.p, b->events ? b->ev_seg.p : nullptr, b->slot_of.p);
    EPH_HIP(hipStreamSynchronize(b->stream));
    return EPH_OK;
}

// SpacecraftPropagator: Clone (the UI snapshots a propagator and later resumes from the snapshot,
// ephemeris_explorer/src/prediction.rs:224-229,378): a deep copy of every per-craft buffer, knots and events included
int32_t eph_craft_batch_clone(eph_craft_batch *b, eph_craft_batch **out) {
    EPH_GUARD_BEGIN
        if (!b || !out) return EPH_ERR_BAD_ARGUMENT;
        *out = nullptr;
        EPH_HIP(hipSetDevice(b->device));
        EPH_HIP(hipStreamSynchronize(b->stream));
        std::unique_ptr<eph_craft_batch> c;
        int st;
        if ((st = craft_batch_shell(*b, b->n, b->max_knots, c)) || (st = copy_buffers(b, c.get(), c->stream))) return st;
        c->h_slot = b->h_slot; c->h_seg_off = b->h_seg_off; c->h_segs = b->h_segs;
        EPH_HIP(hipStreamSynchronize(c->stream));
        *out = c.release();
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_craft_batch_knot_slabs(eph_craft_batch *b, int32_t first_knot, int32_t n_knots, double *knot_t,
                                   double *knot_y) {
    if (!b || first_knot < 0 || n_knots < 0 || first_knot + n_knots > b->max_knots) return EPH_ERR_BAD_ARGUMENT;
    if (b->n == 0 || n_knots == 0) return EPH_OK;
    EPH_HIP(hipSetDevice(b->device));
    const size_t n = (size_t)b->n;
    if (!b->h_slot.empty()) {
        // lane order -> craft order on the device, in passes of at most 256 MB of knot rows (a full slab of a 5e5-craft sweep is
        // GBs: the reorder must not need a second slab), each pass stored by the kernel straight into the pinned staging buffer
        const size_t row_bytes = sizeof(double) * n;
        const long long rows_per_pass = (long long)std::max<size_t>(1, ((size_t)256 << 20) / row_bytes);
        for (int part = 0; part < 2; ++part) {
            double *dst = part == 0 ? knot_t : knot_y;
            if (!dst) continue;
            const long long rows = (long long)n_knots * (part == 0 ? 1 : 6);
            const double *src = part == 0 ? b->knot_t.p + (size_t)first_knot * n : b->knot_y.p + (size_t)first_knot * 6 * n;
            PinnedStage stage((size_t)std::min(rows, rows_per_pass) * row_bytes);
            if (stage.status()) return stage.status();
            StreamIdleOnExit idle(b->stream);
            for (long long r0 = 0; r0 < rows; r0 += rows_per_pass) {
                const long long nr = std::min(rows_per_pass, rows - r0);
                EPH_LAUNCH("k_rows_to_craft_order", k_rows_to_craft_order, dim3((unsigned)((n + 255) / 256)), dim3(256), b->stream, nr,
                           (long long)n, b->slot_of.p, src + (size_t)r0 * n, static_cast<double *>(stage.dev()));
                EPH_HIP(hipStreamSynchronize(b->stream));
                std::memcpy(dst + (size_t)r0 * n, stage.host(), (size_t)nr * row_bytes);
            }
        }
        return EPH_OK;
    }
    if (knot_t)
        EPH_HIP(hipMemcpy(knot_t, b->knot_t.p + (size_t)first_knot * n, sizeof(double) * n * n_knots, hipMemcpyDeviceToHost));
    if (knot_y)
        EPH_HIP(hipMemcpy(knot_y, b->knot_y.p + (size_t)first_knot * 6 * n, sizeof(double) * 6 * n * n_knots,
                          hipMemcpyDeviceToHost));
    return EPH_OK;
}

int32_t eph_craft_batch_kernel_time(eph_craft_batch *b, double *total_ms) {
    if (!b || !total_ms) return EPH_ERR_BAD_ARGUMENT;
    *total_ms = b->kernel_ms;
    return EPH_OK;
}
void eph_craft_batch_destroy(eph_craft_batch *b) { delete b; }

}  // extern "C"
#pragma GCC visibility pop
