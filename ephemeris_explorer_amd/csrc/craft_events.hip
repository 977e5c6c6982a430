// craft_events.hip -- the spacecraft batch's sphere-of-influence / apsis search: the app's SpacecraftSolout on the knots a sweep wrote.
//
// Mirrors (paths relative to the reference repository root):
//   SpacecraftSolout, SoiTransitions, find_zero_crossing, find_root_bisection, find_soi
//                                                       ephemeris_explorer/src/dynamics/spacecraft.rs:77-221,296-451,525-586
//   CubicHermite::{new, eval, eval_derivative}          ephemeris/src/trajectory.rs:645-697
// A body's position and state vector (UniformSpline::{position, state_vector}) are trajectory_eval.h's.
// glam::DVec3 operations (crate glam 0.30.10, not on disk) are restated from the published crate.
#include <algorithm>

#include "craft_batch.h"
#include "craft_events.h"

namespace eph {

// ------------------------------------------------------------------------------------------------------
// SpacecraftSolout events (the app's solout: ephemeris_explorer/src/dynamics/spacecraft.rs:77-221,296-451,539-586):
// after every accepted step, sphere-of-influence crossings of every body and the apsides relative to the current
// sphere's body are searched on the step's CubicHermite by sign test + bisection (<= 100 halvings, 1e-3 s).
// One thread per craft walks its new segments in order (the transition list is sequential state). Bodies are
// visited in body order (the reference iterates an EntityHashMap, whose order is unspecified).
// ------------------------------------------------------------------------------------------------------
struct Hermite { double b0; V3 a0, a1, a2, a3; };
__device__ __forceinline__ V3 hermite_pos(const Hermite &h, double t) {      // CubicHermite::eval  trajectory.rs:681-688
    const double dt = t - h.b0;
    return add(scale(add(scale(add(scale(h.a3, dt), h.a2), dt), h.a1), dt), h.a0);
}
__device__ __forceinline__ V3 hermite_vel(const Hermite &h, double t) {      // eval_derivative :690-697
    const double dt = t - h.b0;
    return add(scale(add(scale(scale(h.a3, dt), 3.0), scale(h.a2, 2.0)), dt), h.a1);
}
// soi_distance_squared_at :77-83 (RADIAL = false) / radial_velocity_at :85-89 (RADIAL = true)
template <bool RADIAL>
__device__ __forceinline__ bool event_f(const EventArgs &a, const Hermite &h, int body, double t, double &out) {
    if (!RADIAL) {
        V3 bp;
        if (!body_position(a.table, body, t, bp)) return false;
        const V3 d = sub(hermite_pos(h, t), bp);
        const double r = a.soi[body];
        out = dot(d, d) - r * r;
        return true;
    }
    V3 bp, bv;
    if (!body_state_vector(a.table, body, t, bp, bv)) return false;
    const V3 rp = sub(hermite_pos(h, t), bp), rv = sub(hermite_vel(h, t), bv);
    out = dot(rp, rv);
    return true;
}
__device__ __forceinline__ double f64_signum(double x) { return x != x ? x : copysign(1.0, x); }
// find_zero_crossing + find_root_bisection :112-162
template <bool RADIAL>
__device__ bool find_zero_crossing(const EventArgs &a, const Hermite &h, int body, double t0, double t1, double &time,
                                   bool &ascending) {
    double f0, f1;
    if (!event_f<RADIAL>(a, h, body, t0, f0) || !event_f<RADIAL>(a, h, body, t1, f1)) return false;
    if (f64_signum(f0) == f64_signum(f1)) return false;
    double x0 = t0, x1 = t1, g0 = f0;
    for (int it = 0; it < 100; ++it) {
        const double mid = x0 + (x1 - x0) / 2.0;
        double f_mid = 0.0;
        event_f<RADIAL>(a, h, body, mid, f_mid);
        if (f64_signum(g0) != f64_signum(f_mid)) x1 = mid;
        else { x0 = mid; g0 = f_mid; }
        if (fabs(x1 - x0) < 1e-3) {
            time = x0;
            ascending = __builtin_signbit(f0);
            return true;
        }
    }
    return false;
}
__device__ bool ap_insert(const EventArgs &a, long long i, int &nap, double time, double dist, int body, int kind) {
    const long long n = a.n_craft;
    int lo = 0, hi = nap;
    bool found = false;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const double tm = a.ap_time[(long long)mid * n + i];
        if (tm == time) { lo = mid; found = true; break; }
        if (tm < time) lo = mid + 1; else hi = mid;
    }
    if (!found) {
        if (nap >= a.max_ap) return false;
        for (int k = nap; k > lo; --k) {
            a.ap_time[(long long)k * n + i] = a.ap_time[(long long)(k - 1) * n + i];
            a.ap_dist[(long long)k * n + i] = a.ap_dist[(long long)(k - 1) * n + i];
            a.ap_body[(long long)k * n + i] = a.ap_body[(long long)(k - 1) * n + i];
            a.ap_kind[(long long)k * n + i] = a.ap_kind[(long long)(k - 1) * n + i];
        }
        nap += 1;
    }
    a.ap_time[(long long)lo * n + i] = time;
    a.ap_dist[(long long)lo * n + i] = dist;
    a.ap_body[(long long)lo * n + i] = body;
    a.ap_kind[(long long)lo * n + i] = kind;
    return true;
}
// WAVE = true (few spacecraft): one wave per craft, every lane in the same state; the sign tests of the SOI search
// -- two body evaluations per body and step, almost never followed by a crossing -- run with lane b on body b, and
// only the bodies whose sign changes go through the (wave-uniform) bisection, in body order.
template <bool WAVE>
__global__ void __launch_bounds__(64) k_craft_events(const EventArgs a) {
    const long long i = WAVE ? (long long)blockIdx.x : (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_craft) return;
    const long long n = a.n_craft;
    if (a.ev_status[i] != EPH_OK) return;
    int seg = a.ev_seg[i], ntr = a.ntr[i], nap = a.nap[i];
    const int nk = a.nknots[i];
    bool full = false;
    const long long col = a.slot_of ? a.slot_of[i] : i;
    auto knot = [&](int k, int d) { return a.knot_y[((long long)k * 6 + d) * n + col]; };
    if (seg < 0) {                                    // new_solution :525-537: the sphere the craft starts in
        const int cur = soi_at_except(a, a.knot_t[col], V3{knot(0, 0), knot(0, 1), knot(0, 2)}, -1);
        if (cur >= 0) full = !tr_insert(a, i, ntr, a.knot_t[col], cur);
        seg = 0;
    }
    for (; !full && seg + 1 < nk; ++seg) {            // solout :539-586 for the step that produced knot seg + 1
        // a slab counts as full while fewer than two entries are free at a step boundary, so that draining
        // (eph_craft_batch_reset_events) resumes exactly at a step; a step needing more than that (several
        // crossings at once into a nearly full slab) still reports EVENTS_FULL, from inside the step
        if (ntr + 2 > a.max_tr || nap + 2 > a.max_ap) { full = true; break; }
        const double t0 = a.knot_t[(long long)seg * n + col], t1 = a.knot_t[(long long)(seg + 1) * n + col];
        const V3 p0 = {knot(seg, 0), knot(seg, 1), knot(seg, 2)}, d0 = {knot(seg, 3), knot(seg, 4), knot(seg, 5)};
        const V3 p1 = {knot(seg + 1, 0), knot(seg + 1, 1), knot(seg + 1, 2)};
        const V3 d1 = {knot(seg + 1, 3), knot(seg + 1, 4), knot(seg + 1, 5)};
        Hermite h;                                    // CubicHermite::new  trajectory.rs:645-679
        h.b0 = t0; h.a0 = p0; h.a1 = d0;
        const double dt = t1 - t0;
        if (dt == 0.0 && p0.x == p1.x && p0.y == p1.y && p0.z == p1.z && d0.x == d1.x && d0.y == d1.y && d0.z == d1.z) {
            h.a2 = {0.0, 0.0, 0.0};
            h.a3 = {0.0, 0.0, 0.0};
        } else {
            const double dt_recip = 1.0 / dt;
            const double dt_recip_2 = dt_recip * dt_recip;
            const double dt_recip_3 = dt_recip * dt_recip_2;
            const V3 dt_val = sub(p1, p0);
            h.a2 = sub(scale(scale(dt_val, dt_recip_2), 3.0), scale(add(scale(d0, 2.0), d1), dt_recip));
            h.a3 = add(scale(scale(dt_val, dt_recip_3), -2.0), scale(add(d0, d1), dt_recip_2));
        }
        auto crossing = [&](int b) {                   // one body's find_soi_crossing and its consequence
            double time;
            bool asc;
            if (!find_zero_crossing<false>(a, h, b, t0, t1, time, asc)) return;
            if (!asc) full = !tr_insert(a, i, ntr, time, b);      // Descending: entered b's sphere
            else {
                const int entered = soi_at_except(a, time, hermite_pos(h, time), b);
                if (entered >= 0) full = !tr_insert(a, i, ntr, time, entered);
            }
        };
        if (WAVE) {
            for (int b0 = 0; b0 < a.n_bodies && !full; b0 += kTile) {
                const int b = b0 + (int)threadIdx.x;
                bool cross = false;
                if (b < a.n_bodies) {                  // the sign test of find_zero_crossing, lane b on body b
                    double f0, f1;
                    cross = event_f<false>(a, h, b, t0, f0) && event_f<false>(a, h, b, t1, f1) &&
                            f64_signum(f0) != f64_signum(f1);
                }
                unsigned long long mask = __builtin_amdgcn_ballot_w64(cross);
                while (mask && !full) {                // body order
                    const int lb = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    crossing(b0 + lb);
                }
            }
        } else {
            for (int b = 0; b < a.n_bodies && !full; ++b) crossing(b);
        }
        if (full) break;
        int lo = 0, hi = ntr, i0 = -1;                // transitions.starting_at(t0) :326-329
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const double tm = a.tr_time[(long long)mid * n + i];
            if (tm == t0) { i0 = mid; break; }
            if (tm < t0) lo = mid + 1; else hi = mid;
        }
        if (i0 < 0) i0 = lo == 0 ? 0 : lo - 1;
        for (int q = i0; q < ntr && !full; ++q) {
            const double t = a.tr_time[(long long)q * n + i];
            const int soi = a.tr_body[(long long)q * n + i];
            const double ta = t0 > t ? t0 : t;
            const double tb = q + 1 < ntr ? a.tr_time[(long long)(q + 1) * n + i] : t1;
            double time;
            bool asc;
            if (!find_zero_crossing<true>(a, h, soi, ta, tb, time, asc)) continue;
            V3 bp;
            if (!body_position(a.table, soi, time, bp)) continue;
            const V3 d = sub(bp, hermite_pos(h, time));          // distance_at  dynamics/mod.rs:141-146
            full = !ap_insert(a, i, nap, time, sqrt(dot(d, d)), soi, asc ? 0 : 1);
        }
        if (full) break;
    }
    a.ev_seg[i] = seg;
    a.ntr[i] = ntr;
    a.nap[i] = nap;
    if (full) a.ev_status[i] = EPH_EVENTS_FULL;
}

// eph_craft_batch_reset_events: keeps the newest transition (the sphere the craft is in -- what
// SoiTransitions::starting_at needs for the next step), drops the older ones and all apsides, clears EVENTS_FULL
__global__ void __launch_bounds__(256) k_craft_reset_events(long long n, int *ntr, int *nap, int *ev_status,
                                                            double *tr_time, int *tr_body) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = ntr[i];
    if (k > 1) {
        tr_time[i] = tr_time[(long long)(k - 1) * n + i];
        tr_body[i] = tr_body[(long long)(k - 1) * n + i];
        ntr[i] = 1;
    }
    nap[i] = 0;
    if (ev_status[i] == EPH_EVENTS_FULL) ev_status[i] = EPH_OK;
}

// craft_run's event step: the search over the steps just taken, queued on `s` behind the sweep
int craft_events_search(eph_craft_batch *b, hipStream_t s) {
    const EventArgs e = event_args(b);
    if (craft_wave_form(b->n)) EPH_LAUNCH("k_craft_events", k_craft_events<true>, dim3((unsigned)b->n), dim3(64), s, e);
    else EPH_LAUNCH("k_craft_events", k_craft_events<false>, dim3((unsigned)((b->n + 63) / 64)), dim3(64), s, e);
    return EPH_OK;
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_enable_events(eph_craft_batch *b, const double *soi_radius, int32_t max_transitions,
                                      int32_t max_apsides) {
    EPH_GUARD_BEGIN
        if (!b || !soi_radius || max_transitions < 1 || max_apsides < 1 || b->events) return EPH_ERR_BAD_ARGUMENT;
        EPH_HIP(hipSetDevice(b->device));
        const size_t nn = (size_t)std::max<long long>(b->n, 1);
        const int nb = b->eph->n_bodies;
        if (const int st = alloc_events(b, max_transitions, max_apsides)) return st;
        if (nb) EPH_HIP(hipMemcpy(b->soi.p, soi_radius, sizeof(double) * nb, hipMemcpyHostToDevice));
        EPH_HIP(hipMemset(b->ev_seg.p, 0xff, sizeof(int) * nn));       // -1: new_solution pending
        EPH_HIP(hipMemset(b->ntr.p, 0, sizeof(int) * nn));
        EPH_HIP(hipMemset(b->nap.p, 0, sizeof(int) * nn));
        EPH_HIP(hipMemset(b->ev_status.p, 0, sizeof(int) * nn));
        b->max_tr = max_transitions;
        b->max_ap = max_apsides;
        b->events = true;
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_craft_batch_event_counts(eph_craft_batch *b, int32_t *n_transitions, int32_t *n_apsides,
                                     int32_t *event_status) {
    if (!b || !b->events) return EPH_ERR_BAD_ARGUMENT;
    EPH_HIP(hipSetDevice(b->device));
    const size_t n = (size_t)b->n;
    if (n == 0) return EPH_OK;
    if (n_transitions) EPH_HIP(hipMemcpy(n_transitions, b->ntr.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (n_apsides) EPH_HIP(hipMemcpy(n_apsides, b->nap.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (event_status) EPH_HIP(hipMemcpy(event_status, b->ev_status.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    return EPH_OK;
}

int32_t eph_craft_batch_events(eph_craft_batch *b, int64_t craft, double *tr_time, int32_t *tr_body, double *ap_time,
                               double *ap_distance, int32_t *ap_body, int32_t *ap_kind) {
    if (!b || !b->events || craft < 0 || craft >= b->n) return EPH_ERR_BAD_ARGUMENT;
    EPH_HIP(hipSetDevice(b->device));
    int ntr = 0, nap = 0;
    EPH_HIP(hipMemcpy(&ntr, b->ntr.p + craft, sizeof(int), hipMemcpyDeviceToHost));
    EPH_HIP(hipMemcpy(&nap, b->nap.p + craft, sizeof(int), hipMemcpyDeviceToHost));
    const long long n = b->n;
#define EPH_COLUMN(dst, src, T, cnt)                                                                             \
    if ((dst) && (cnt) > 0)                                                                                      \
        EPH_HIP(hipMemcpy2D((dst), sizeof(T), (src) + craft, sizeof(T) * n, sizeof(T), (cnt), hipMemcpyDeviceToHost))
    EPH_COLUMN(tr_time, b->tr_time.p, double, ntr);
    EPH_COLUMN(tr_body, b->tr_body.p, int, ntr);
    EPH_COLUMN(ap_time, b->ap_time.p, double, nap);
    EPH_COLUMN(ap_distance, b->ap_dist.p, double, nap);
    EPH_COLUMN(ap_body, b->ap_body.p, int, nap);
    EPH_COLUMN(ap_kind, b->ap_kind.p, int, nap);
#undef EPH_COLUMN
    return EPH_OK;
}

int32_t eph_craft_batch_reset_events(eph_craft_batch *b) {
    if (!b || !b->events) return EPH_ERR_BAD_ARGUMENT;
    if (b->n == 0) return EPH_OK;
    EPH_HIP(hipSetDevice(b->device));
    EPH_LAUNCH("k_craft_reset_events", k_craft_reset_events, dim3((unsigned)((b->n + 255) / 256)), dim3(256), b->stream, b->n,
               b->ntr.p, b->nap.p, b->ev_status.p, b->tr_time.p, b->tr_body.p);
    EPH_HIP(hipStreamSynchronize(b->stream));
    return EPH_OK;
}

}  // extern "C"
#pragma GCC visibility pop
