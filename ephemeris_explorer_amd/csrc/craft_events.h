// craft_events.h -- what the event search (craft_events.hip) shares with the flight-plan restart (craft_restart.hip): the search's
// argument block, find_soi and SoiTransitions::insert on a craft's column of the slabs.
// Mirrors ephemeris_explorer/src/dynamics/spacecraft.rs:172-185,208-221,332-339 (paths relative to the reference repository root).
#pragma once
#include "craft_batch.h"

namespace eph {

struct EventArgs {
    long long n_craft;
    int n_bodies;
    BodyTable table;              // the live table (trajectory_eval.h)
    const double *soi;            // [n_bodies] sphere radii (inf for the root)
    const int *nknots;
    const double *knot_t, *knot_y;
    int *ev_seg;                  // next segment (knot pair k, k+1) to examine; -1 = new_solution not yet run
    int *ntr, *nap, *ev_status;
    double *tr_time; int *tr_body;                              // [max_tr][n]
    double *ap_time, *ap_dist; int *ap_body, *ap_kind;          // [max_ap][n]
    int max_tr, max_ap;
    const int *slot_of;           // craft -> its column in the knot slabs (null: identity)
};
// the batch's event slabs and the live table; a batch without events has null slabs (the restart reads find_soi's table only)
inline EventArgs event_args(const eph_craft_batch *b) {
    EventArgs e{};
    e.n_craft = b->n; e.n_bodies = b->eph->n_bodies;
    e.table = body_table(b->eph);
    e.soi = b->soi.p; e.nknots = b->nknots.p; e.knot_t = b->knot_t.p; e.knot_y = b->knot_y.p;
    e.ev_seg = b->ev_seg.p; e.ntr = b->ntr.p; e.nap = b->nap.p; e.ev_status = b->ev_status.p;
    e.tr_time = b->tr_time.p; e.tr_body = b->tr_body.p;
    e.ap_time = b->ap_time.p; e.ap_dist = b->ap_dist.p; e.ap_body = b->ap_body.p; e.ap_kind = b->ap_kind.p;
    e.max_tr = b->max_tr; e.max_ap = b->max_ap;
    e.slot_of = b->slot_of.p;
    return e;
}
// find_soi :172-185,208-221: inside iff d2 < r*r; the closest wins, the first on ties
__device__ inline int soi_at_except(const EventArgs &a, double t, V3 position, int except) {
    int best = -1;
    double best_d2 = 0.0;
    for (int b = 0; b < a.n_bodies; ++b) {
        if (b == except) continue;
        V3 bp;
        if (!body_position(a.table, b, t, bp)) continue;
        const V3 d = sub(position, bp);
        const double d2 = dot(d, d), r = a.soi[b];
        if (!(d2 < r * r)) continue;
        if (best < 0 || d2 < best_d2) { best = b; best_d2 = d2; }
    }
    return best;
}
// SoiTransitions::insert :332-339 on the craft's column of the slab; false = slab full
__device__ inline bool tr_insert(const EventArgs &a, long long i, int &ntr, double time, int body) {
    const long long n = a.n_craft;
    int lo = 0, hi = ntr;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const double tm = a.tr_time[(long long)mid * n + i];
        if (tm == time) { a.tr_body[(long long)mid * n + i] = body; return true; }
        if (tm < time) lo = mid + 1; else hi = mid;
    }
    if (lo > 0 && a.tr_body[(long long)(lo - 1) * n + i] == body) return true;
    if (ntr >= a.max_tr) return false;
    for (int k = ntr; k > lo; --k) {
        a.tr_time[(long long)k * n + i] = a.tr_time[(long long)(k - 1) * n + i];
        a.tr_body[(long long)k * n + i] = a.tr_body[(long long)(k - 1) * n + i];
    }
    a.tr_time[(long long)lo * n + i] = time;
    a.tr_body[(long long)lo * n + i] = body;
    ntr += 1;
    return true;
}
}  // namespace eph
