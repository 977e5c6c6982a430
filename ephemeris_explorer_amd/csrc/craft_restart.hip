// craft_restart.hip -- flight-plan restart of a spacecraft batch in place (eph_craft_batch_restart): every selected craft continues
// from the knot where its new flight plan diverges from the old one, as the app's new propagator would, merged into what it holds.
//
// Mirrors (paths relative to the reference repository root):
//   FlightPlan::restart_propagator, apply_flight_plan   ephemeris_explorer/src/flight_plan.rs:263-303,325-361
//   Timeline::{common_times, divergence_time_before}    ephemeris/src/propagators/spacecraft.rs:179-213
//   CubicHermiteSpline::get (exact knot lookup)         ephemeris/src/trajectory.rs:846-849
//   SpacecraftPropagator::new, from_problem             ephemeris/src/propagators/spacecraft.rs:58-152
//   PredictionTarget::merge, SpacecraftSolout::new_solution
//                                                       ephemeris_explorer/src/dynamics/spacecraft.rs:523-537,830-841
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "craft_batch.h"
#include "craft_events.h"

namespace eph {

constexpr int kRestartSkipped = 0x7fffffff;   // outcome of an unselected craft inside the staging buffer (never given to the caller)

struct RestartArgs {
    long long n;
    const uint8_t *which;                     // [craft] or null: every craft
    const long long *old_off;                 // the batch's CSR timelines
    const SegmentDev *old_segs;
    const long long *new_off;                 // the new flight plans (empty for unselected craft)
    const SegmentDev *new_segs;
    const double *plan_end;                   // [craft] or null: +inf
    const double *t_start;                    // [craft] creation epoch = trajectory.start()
    int params_changed;                       // tolerance or n_max differ: restart at the trajectory start
    double h_init;
    const int *slot_of;                       // craft -> knot-slab column (null: identity)
    const double *knot_t, *knot_y;
    double *time, *y, *next_h, *klast, *kfirst, *last_knot;
    unsigned *n_attempts, *rk_i;
    int *cur_seg, *status, *nknots;
    int events;
    EventArgs ev;                             // event slabs (events != 0) and the live table for find_soi
    double *epoch_out;                        // [craft] into the pinned staging buffer
    int *outcome_out;
};

// one lane per craft: the restart epoch, the exact knot, then -- only once nothing can fail any more -- the new propagator's state
// and the merged event lists. A craft that does not restart is left bit for bit as it was.
__global__ void __launch_bounds__(256) k_craft_restart(const RestartArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const long long n = a.n;
    if (a.which && !a.which[i]) { a.outcome_out[i] = kRestartSkipped; return; }
    const long long col = a.slot_of ? a.slot_of[i] : i;
    const int nk = a.nknots[i];
    const double t_start = a.t_start[i];
    double epoch;
    if (a.params_changed) {
        epoch = t_start;                                           // flight_plan.rs:283-287
    } else {
        const double end = a.knot_t[(long long)(nk - 1) * n + col];   // trajectory.end()
        const double before = a.plan_end ? (a.plan_end[i] <= end ? a.plan_end[i] : end) : end;   // self.end.min(trajectory.end())
        // divergence_time_before: self = the new timeline, zipped with the old one while the segment starts agree, stopping after the
        // first pair whose thrust differs; the last such start that is < before
        const SegmentDev *sa = a.new_segs + a.new_off[i], *sb = a.old_segs + a.old_off[i];
        const long long na = a.new_off[i + 1] - a.new_off[i], nb = a.old_off[i + 1] - a.old_off[i];
        bool done = false, any = false;
        double last = 0.0;
        for (long long k = 0; k < na && k < nb; ++k) {
            const SegmentDev s1 = sa[k], s2 = sb[k];
            if (done || s1.start != s2.start) break;
            const bool same = s1.is_burn == s2.is_burn &&
                              (!s1.is_burn || (s1.ax == s2.ax && s1.ay == s2.ay && s1.az == s2.az && s1.ref == s2.ref));
            if (!same) done = true;
            if (!(s1.start < before)) break;
            last = s1.start;
            any = true;
        }
        if (!any) {                                                // the reference's unwrap
            a.epoch_out[i] = __builtin_nan("");
            a.outcome_out[i] = EPH_ERR_BAD_ARGUMENT;
            return;
        }
        epoch = last > t_start ? last : t_start;                   // .max(trajectory.start())
    }
    a.epoch_out[i] = epoch;
    int lo = 0, hi = nk, j = -1;                                   // trajectory.get(restart_epoch): binary search, exact match
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const double tm = a.knot_t[(long long)mid * n + col];
        if (tm == epoch) { j = mid; break; }
        if (tm < epoch) lo = mid + 1; else hi = mid;
    }
    if (j < 0) { a.outcome_out[i] = EPH_EVAL_FAILED; return; }
    double sv[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) sv[d] = a.knot_y[((long long)j * 6 + d) * n + col];
    int keep_tr = 0, keep_ap = 0, soi = -1;
    if (a.events) {
        // the steps before knot j must have been searched: their events are what the merge keeps
        const int seg = a.ev.ev_seg[i];
        if (seg < j && !(seg < 0 && j == 0)) { a.outcome_out[i] = EPH_EVENTS_FULL; return; }
        const int ntr = a.ev.ntr[i], nap = a.ev.nap[i];
        // clear_after(epoch): the entries with t <= epoch (times are distinct: both inserts replace an equal time)
        lo = 0; hi = ntr;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (a.ev.tr_time[(long long)mid * n + i] <= epoch) lo = mid + 1; else hi = mid;
        }
        keep_tr = lo;
        lo = 0; hi = nap;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (a.ev.ap_time[(long long)mid * n + i] <= epoch) lo = mid + 1; else hi = mid;
        }
        keep_ap = lo;
        soi = soi_at_except(a.ev, epoch, V3{sv[0], sv[1], sv[2]}, -1);      // new_solution's soi_at (LIVE table)
        // SoiTransitions::insert after clear_after: every kept entry is at or before `epoch`, so it replaces an entry AT epoch,
        // is dropped behind an entry of the same body, or takes slot keep_tr -- which must exist
        if (soi >= 0 && keep_tr >= a.ev.max_tr && !(a.ev.tr_time[(long long)(keep_tr - 1) * n + i] == epoch ||
                                                     a.ev.tr_body[(long long)(keep_tr - 1) * n + i] == soi)) {
            a.outcome_out[i] = EPH_EVENTS_FULL;
            return;
        }
    }
    // SpacecraftPropagator::new at (epoch, knot j) with the new timeline and the batch's parameters
    a.time[i] = epoch;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        a.y[d * n + i] = sv[d];
        a.klast[d * n + i] = sv[d];                                // from_problem: k = [state; STAGES]
        a.kfirst[d * n + i] = sv[d];
    }
    a.next_h[i] = a.h_init;
    a.n_attempts[i] = 0;
    a.rk_i[i] = 0;
    const SegmentDev *sa = a.new_segs + a.new_off[i];
    const int ns = (int)(a.new_off[i + 1] - a.new_off[i]);
    int cur = 0;                                                   // segment_idx_at: partition_point(seg.end() <= time)
    while (cur < ns && sa[cur].end <= epoch) ++cur;
    a.cur_seg[i] = cur;
    a.status[i] = EPH_OK;
    // join: knots 0 .. j stay, the new solution's first knot is knot j itself
    a.nknots[i] = j + 1;
    a.last_knot[i] = epoch;
    if (a.events) {
        int ntr = keep_tr;
        if (soi >= 0) (void)tr_insert(a.ev, i, ntr, epoch, soi);
        a.ev.ntr[i] = ntr;
        a.ev.nap[i] = keep_ap;
        a.ev.ev_seg[i] = j;                                        // the search resumes with the step that starts at knot j
        a.ev.ev_status[i] = EPH_OK;
    }
    a.outcome_out[i] = EPH_OK;
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_restart(eph_craft_batch *b, const uint8_t *which, const int64_t *burn_offset, const double *burn_start,
                                const double *burn_end, const double *burn_acc_xyz, const int32_t *burn_ref, const double *plan_end,
                                const eph_adaptive_params *params, double *restart_epoch, int32_t *outcome) {
    EPH_GUARD_BEGIN
        if (!b || (params && which)) return EPH_ERR_BAD_ARGUMENT;
        const long long n = b->n;
        auto selected = [&](long long i) { return !which || which[i] != 0; };
        // validate everything before anything changes: the CSR over all craft, the burns of the selected ones (as create)
        int st = burn_csr_check(n, burn_offset, burn_start, burn_end, burn_acc_xyz, burn_ref, b->eph->n_bodies, which, false);
        if (st || (b->rk.nystrom == 2 && (st = burn_erkn_check(n, burn_offset, burn_ref, which)))) return st;
        const eph_adaptive_params next = params ? *params : b->params;
        // flight_plan.rs:283-285 (the method is the batch's own and cannot change)
        const bool params_changed = next.tol_position != b->params.tol_position || next.tol_velocity != b->params.tol_velocity ||
                                    next.n_max != b->params.n_max;
        if (n == 0) {
            b->params = next;
            return EPH_OK;
        }
        EPH_HIP(hipSetDevice(b->device));
        std::shared_lock<std::shared_mutex> table_lock(b->eph->mu);   // find_soi reads the live table, like a sweep
        EPH_HIP(hipStreamSynchronize(b->stream));
        // Timeline::new of every selected craft's new plan
        std::vector<long long> new_off((size_t)n + 1, 0);
        std::vector<SegmentDev> new_segs;
        for (long long i = 0; i < n; ++i) {
            new_off[(size_t)i] = (long long)new_segs.size();
            if (!selected(i)) continue;
            const long long b0 = burn_offset ? burn_offset[i] : 0, b1 = burn_offset ? burn_offset[i + 1] : 0;
            timeline_new(b1 - b0, burn_start + b0, burn_end + b0, burn_acc_xyz + 3 * b0, burn_ref + b0, new_segs);
        }
        new_off[(size_t)n] = (long long)new_segs.size();
        // every allocation before the kernel: the batch's new CSR cannot need more than old + new segments
        DevBuf<long long> d_new_off;
        DevBuf<SegmentDev> d_new_segs, d_segs;
        DevBuf<uint8_t> d_which;
        DevBuf<double> d_plan_end;
        if ((st = upload(d_new_off, new_off.data(), new_off.size())) || (st = upload(d_new_segs, new_segs.data(), new_segs.size())) ||
            (which && (st = upload(d_which, which, (size_t)n))) || (plan_end && (st = upload(d_plan_end, plan_end, (size_t)n))) ||
            (st = d_segs.alloc(std::max<size_t>(b->h_segs.size() + new_segs.size(), 1))))
            return st;
        PinnedStage stage((size_t)n * (sizeof(double) + sizeof(int)));
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(b->stream);
        RestartArgs a{};
        a.n = n; a.which = which ? d_which.p : nullptr;
        a.old_off = b->seg_off.p; a.old_segs = b->segs.p; a.new_off = d_new_off.p; a.new_segs = d_new_segs.p;
        a.plan_end = plan_end ? d_plan_end.p : nullptr; a.t_start = b->t_start.p;
        a.params_changed = params_changed ? 1 : 0; a.h_init = next.h_init;
        a.slot_of = b->h_slot.empty() ? nullptr : b->slot_of.p;
        a.knot_t = b->knot_t.p; a.knot_y = b->knot_y.p;
        a.time = b->time.p; a.y = b->y.p; a.next_h = b->next_h.p; a.klast = b->klast.p; a.kfirst = b->kfirst.p; a.last_knot = b->last_knot.p;
        a.n_attempts = b->n_attempts.p; a.rk_i = b->rk_i.p; a.cur_seg = b->cur_seg.p; a.status = b->status.p; a.nknots = b->nknots.p;
        a.events = b->events ? 1 : 0;
        a.ev = event_args(b);
        a.epoch_out = static_cast<double *>(stage.dev());
        a.outcome_out = reinterpret_cast<int *>(a.epoch_out + n);
        EPH_LAUNCH("k_craft_restart", k_craft_restart, dim3((unsigned)((n + 255) / 256)), dim3(256), b->stream, a);
        EPH_HIP(hipStreamSynchronize(b->stream));
        idle.disarm();
        const double *h_epoch = stage.host_of(a.epoch_out);
        const int *h_outcome = stage.host_of(a.outcome_out);
        // the batch's CSR: the new timeline for every restarted craft, the old one for everyone else
        std::vector<long long> off((size_t)n + 1, 0);
        std::vector<SegmentDev> segs;
        segs.reserve(b->h_segs.size() + new_segs.size());
        for (long long i = 0; i < n; ++i) {
            off[(size_t)i] = (long long)segs.size();
            const bool fresh = h_outcome[i] == EPH_OK;
            const std::vector<SegmentDev> &src = fresh ? new_segs : b->h_segs;
            const std::vector<long long> &so = fresh ? new_off : b->h_seg_off;
            segs.insert(segs.end(), src.begin() + so[(size_t)i], src.begin() + so[(size_t)i + 1]);
            if (h_outcome[i] == kRestartSkipped) continue;
            if (restart_epoch) restart_epoch[i] = h_epoch[i];
            if (outcome) outcome[i] = h_outcome[i];
        }
        off[(size_t)n] = (long long)segs.size();
        if (!segs.empty()) EPH_HIP(hipMemcpy(d_segs.p, segs.data(), sizeof(SegmentDev) * segs.size(), hipMemcpyHostToDevice));
        EPH_HIP(hipMemcpy(b->seg_off.p, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
        b->segs.swap(d_segs);
        b->h_seg_off = std::move(off);
        b->h_segs = std::move(segs);
        b->params = next;
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
