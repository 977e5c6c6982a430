// craft_markers.hip -- the event markers of a batch's plots (eph_craft_batch_plot_markers): for every plot of a ship, the burn starts,
// SOI transitions, apsides and trajectory bounds of that ship that fall inside the plot's points, each with relative.position(t),
// its length and, for a burn, the TNB frame at the burn's start. Reads the batch; changes nothing in it.
//
// Mirrors (paths relative to the reference repository root):
//   plot_manoeuvre_markers, plot_transition_markers, plot_apsis_markers, plot_bounds_markers
//                                                                     ephemeris_explorer/src/ui/world/tooltip.rs:84-245
//   manoeuvre_marker_picking, transition_marker_picking, apsis_marker_picking, bound_marker_picking
//                                                                     ephemeris_explorer/src/ui/world/picking.rs:256-447
//   PlotPoints::contains                                              ephemeris_explorer/src/ui/world/plot.rs:170-173
//   RelativeTrajectory::position, CubicHermiteSpline::position        ephemeris/src/trajectory.rs:319-325,784-789
//   TNB::try_new, ReferenceFrame::transform                           ephemeris_explorer/src/dynamics/spacecraft.rs:240-293
// The trajectory evaluations are trajectory_eval.h's. TNB::try_new is restated here, operation for operation as burn_acceleration
// (craft_sweep.hip) states it inside the tuned sweep kernels, which stay as they are.
//
// Three steps, the shape of k_craft_plot_segments: COUNT, one lane per request -- the transition slab, the apsis slab and the
// timeline's starts are sorted by time, so a request's candidates in each list are the range between two bound searches, kept in a
// MarkerRanges for the fill; one integer per request comes back through the pinned staging buffer and the host does the prefix sums.
// FILL, one lane per MARKER: a ship in a low orbit collects thousands of apsides beside neighbours with a handful, and each record is a
// binary search of a knot column, a cubic and a body Horner; a lane finds its request by an upper-bound search of the prefix sum.
// Requests are ordered by slab column (LaneMap), so neighbouring markers read the same column. OUT: records go to a device block in
// lane order, travel through the staging pool, and the host moves each request's run to its place in the caller's array.
#include <algorithm>
#include <climits>
#include <cstring>

#include "craft_batch.h"
#include "craft_events.h"

namespace eph {

struct MarkerRanges {         // one request's candidates: first index and count in each list, and which bounds
    int seg0, n_burn;               // timeline segments from seg0 on (of the craft's slice of the CSR): the first n_burn burns
    int tr0, n_tr;
    int ap0, n_ap;
    int bounds, total;              // bit 0 Start, bit 1 End
};
struct CraftMarkerArgs {
    long long n_lanes;              // requests
    const long long *lane_item;     // lane -> request; lanes are ordered by slab column
    const int *lane_col;            // lane -> slab column of the request's craft
    const eph_marker_request *req;  // [request]
    const long long *craft;         // [request], null: request r is craft r
    KnotSlabs slabs;
    EventArgs ev;                   // the event slabs ([k][craft]; max_tr = 0: a batch without events) and the live table
    const long long *seg_off;       // the timeline CSR
    const SegmentDev *segs;
    MarkerRanges *ranges;           // [lane]
    int *count;                     // the count step: records per lane (pinned)
    const long long *lane_first;    // the fill step: [lanes + 1] exclusive prefix sum of the counts, lane order
    long long m0, m1;               // the fill step: markers [m0, m1) of the call, record m at out[m - m0]
    eph_plot_marker *out;
};

// the first k in [0, n) with at(k) >= x (UPPER: > x); at(k) never decreases
template <bool UPPER, class At>
__device__ __forceinline__ int bound_search(int n, double x, At at) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const double tm = at(mid);
        if (UPPER ? tm <= x : tm < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// PlotPoints::contains plot.rs:170-173
__device__ __forceinline__ bool contains(const eph_marker_request &rq, double t) { return rq.first <= t && rq.last >= t; }

__global__ void __launch_bounds__(64) k_craft_markers_count(const CraftMarkerArgs a) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= a.n_lanes) return;
    const long long r = a.lane_item[lane];
    const eph_marker_request rq = a.req[r];
    const long long c = a.craft ? a.craft[r] : r, n = a.ev.n_craft;
    MarkerRanges g = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rq.kinds & 1) {                                 // the burns whose start the window contains
        const SegmentDev *segs = a.segs + a.seg_off[c];
        const int nseg = (int)(a.seg_off[c + 1] - a.seg_off[c]);
        g.seg0 = bound_search<false>(nseg, rq.first, [&](int k) { return segs[k].start; });
        const int seg1 = bound_search<true>(nseg, rq.last, [&](int k) { return segs[k].start; });
        for (int k = g.seg0; k < seg1; ++k) g.n_burn += segs[k].is_burn ? 1 : 0;
    }
    if ((rq.kinds & 2) && a.ev.max_tr > 0) {
        const int ntr = min(max(a.ev.ntr[c], 0), a.ev.max_tr);
        g.tr0 = bound_search<false>(ntr, rq.first, [&](int k) { return a.ev.tr_time[(long long)k * n + c]; });
        g.n_tr = max(bound_search<true>(ntr, rq.last, [&](int k) { return a.ev.tr_time[(long long)k * n + c]; }) - g.tr0, 0);
    }
    if ((rq.kinds & 4) && a.ev.max_ap > 0) {
        const int nap = min(max(a.ev.nap[c], 0), a.ev.max_ap);
        g.ap0 = bound_search<false>(nap, rq.first, [&](int k) { return a.ev.ap_time[(long long)k * n + c]; });
        g.n_ap = max(bound_search<true>(nap, rq.last, [&](int k) { return a.ev.ap_time[(long long)k * n + c]; }) - g.ap0, 0);
    }
    if (rq.kinds & 8) {                                 // trajectory.start() / .end(): the first and the last knot
        const KnotColumn kn = a.slabs.column(a.lane_col[lane], c);
        if (kn.nk > 0) g.bounds = (contains(rq, kn.t(0)) ? 1 : 0) | (contains(rq, kn.t(kn.nk - 1)) ? 2 : 0);
    }
    g.total = g.n_burn + g.n_tr + g.n_ap + (g.bounds & 1) + (g.bounds >> 1);
    a.ranges[lane] = g;
    a.count[lane] = g.total;
}

// One marker per lane. 144 bytes a record, every field written (the struct has no padding).
__global__ void __launch_bounds__(64) k_craft_markers_fill(const CraftMarkerArgs a) {
    const long long m = a.m0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.m1) return;
    long long lo = 0, hi = a.n_lanes;                   // the lane with lane_first[lane] <= m < lane_first[lane + 1]
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (a.lane_first[mid + 1] <= m) lo = mid + 1; else hi = mid;
    }
    const long long lane = lo;
    if (lane >= a.n_lanes) return;                      // (m < lane_first[n_lanes]: never)
    const long long r = a.lane_item[lane];
    const eph_marker_request rq = a.req[r];
    const long long c = a.craft ? a.craft[r] : r, n = a.ev.n_craft;
    const MarkerRanges g = a.ranges[lane];
    const KnotColumn kn = a.slabs.column(a.lane_col[lane], c);
    int j = (int)(m - a.lane_first[lane]);
    int kind, index = 0, body = -1, burn_ref = -1;
    double t, apsis_distance = 0.0;
    if (j < g.n_burn) {                                 // the j-th burn from seg0 on
        const SegmentDev *segs = a.segs + a.seg_off[c];
        const int nseg = (int)(a.seg_off[c + 1] - a.seg_off[c]);
        int k = g.seg0;
        for (int seen = -1; k < nseg; ++k) {
            seen += segs[k].is_burn ? 1 : 0;
            if (seen == j) break;
        }
        if (k >= nseg) return;                          // (the count step found n_burn of them: never)
        kind = 0; index = k; t = segs[k].start; burn_ref = segs[k].ref; body = burn_ref;
    } else if ((j -= g.n_burn) < g.n_tr) {
        const long long at = (long long)(g.tr0 + j) * n + c;
        kind = 1; index = g.tr0 + j; t = a.ev.tr_time[at]; body = a.ev.tr_body[at];
    } else if ((j -= g.n_tr) < g.n_ap) {
        const long long at = (long long)(g.ap0 + j) * n + c;
        kind = a.ev.ap_kind[at] ? 3 : 2; index = g.ap0 + j; t = a.ev.ap_time[at]; body = a.ev.ap_body[at];
        apsis_distance = a.ev.ap_dist[at];
    } else {
        j -= g.n_ap;
        if (kn.nk <= 0) return;                         // (a bound was counted: never)
        const bool start = (g.bounds & 1) && j == 0;
        kind = start ? 4 : 5;
        t = start ? kn.t(0) : kn.t(kn.nk - 1);
    }
    int status = 0;
    V3 position = {0.0, 0.0, 0.0};
    double distance = 0.0, frame[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // RelativeTrajectory::position trajectory.rs:319-325: the reference's position (Default without one), then the craft's
    V3 rp = {0.0, 0.0, 0.0}, sp, sv;
    const bool ref_ok = rq.reference_body < 0 || body_position(a.ev.table, rq.reference_body, t, rp);
    const bool craft_ok = hermite_state_vector(kn, t, sp, sv);
    if (ref_ok && craft_ok) {
        position = sub(sp, rp);
        distance = sqrt(dot(position, position));       // glam length: sqrt((x*x + y*y) + z*z)
        status |= 1;
    }
    // trajectory.state_vector(burn.start).and_then(|sv| burn.reference_frame().transform(burn.start, &sv, ..))  tooltip.rs:105-108
    if (kind == 0 && craft_ok) {
        if (burn_ref < 0) {                             // TNB::IDENTITY
            frame[0] = frame[4] = frame[8] = 1.0;
            status |= 2;
        } else {                                        // TNB::try_new(sv - body.state_vector(t))  spacecraft.rs:247-252,287-289
            V3 bp, bv, x, y;
            if (body_state_vector(a.ev.table, burn_ref, t, bp, bv)) {
                const V3 rel_p = sub(sp, bp), rel_v = sub(sv, bv);
                if (try_normalize(rel_v, x) && try_normalize(cross(rel_p, rel_v), y)) {
                    const V3 xy = cross(x, y);
                    const V3 z = scale(xy, length_recip(xy));
                    frame[0] = x.x; frame[1] = x.y; frame[2] = x.z;         // DMat3::from_cols(x, z, y)
                    frame[3] = z.x; frame[4] = z.y; frame[5] = z.z;
                    frame[6] = y.x; frame[7] = y.y; frame[8] = y.z;
                    status |= 2;
                }
            }
        }
    }
    eph_plot_marker *o = a.out + (m - a.m0);
    o->request = r; o->kind = kind; o->index = index; o->body = body; o->status = status;
    o->time = t;
    o->position[0] = position.x; o->position[1] = position.y; o->position[2] = position.z;
    o->distance = distance;
    o->apsis_distance = apsis_distance;
#pragma unroll
    for (int q = 0; q < 9; ++q) o->frame[q] = frame[q];
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_plot_markers(eph_craft_batch *b, int64_t n_requests, const eph_marker_request *requests,
                                     const int64_t *craft, int64_t marker_capacity, eph_plot_marker *out_markers,
                                     int64_t *out_first) {
    EPH_GUARD_BEGIN
        static_assert(sizeof(eph_marker_request) == 24 && sizeof(eph_plot_marker) == 144, "the C layouts");
        if (!b || n_requests < 0 || marker_capacity < 0 || (marker_capacity > 0 && !out_markers) ||
            (n_requests > 0 && (!requests || !out_first)))
            return EPH_ERR_BAD_ARGUMENT;
        const int nb = b->eph->n_bodies;
        const size_t nr = (size_t)n_requests;
        if (!craft && n_requests > b->n) return EPH_ERR_BAD_ARGUMENT;
        bool reads_table = false;
        for (size_t r = 0; r < nr; ++r) {
            const eph_marker_request &q = requests[r];
            if (q.reference_body < -1 || q.reference_body >= nb || q.kinds < 0 || q.kinds > 15 || q.first != q.first || q.last != q.last ||
                (craft && (craft[r] < 0 || craft[r] >= b->n)))
                return EPH_ERR_BAD_ARGUMENT;
            reads_table = reads_table || q.reference_body >= 0;
        }
        if (n_requests == 0 || b->n == 0) return EPH_OK;
        // a candidate burn in a relative frame reads its body's state vector: the host's mirror of the timelines tells
        for (size_t r = 0; r < nr && !reads_table; ++r) {
            const eph_marker_request &q = requests[r];
            const size_t c = craft ? (size_t)craft[r] : r;
            for (long long k = b->h_seg_off[c]; (q.kinds & 1) && k < b->h_seg_off[c + 1] && !reads_table; ++k) {
                const SegmentDev &sg = b->h_segs[(size_t)k];
                reads_table = sg.is_burn && sg.ref >= 0 && q.first <= sg.start && q.last >= sg.start;
            }
        }
        LaneMap lanes;                                  // lanes in slab-column order
        int st;
        if ((st = lanes.sort(b, nr, craft))) return st;
        const auto table_lock = table_lock_if(b->eph, reads_table);
        EPH_HIP(hipSetDevice(b->device));
        // kernel time and host time of the two steps (scripts/craft_markers_timing.py): the count with the host's scans, the fill with
        // the moves into the caller's array
        PassTrace count_trace("EPH_TRACE_CRAFT_MARKERS", b), trace("EPH_TRACE_CRAFT_MARKERS", b);
        hipStream_t s = b->stream;
        DevBuf<eph_marker_request> d_req;
        DevBuf<long long> d_craft, d_first;
        DevBuf<MarkerRanges> d_ranges;
        if ((st = d_req.alloc(nr)) || (st = d_craft.alloc(craft ? nr : 0)) || (st = d_first.alloc(nr + 1)) || (st = d_ranges.alloc(nr)))
            return st;
        CraftMarkerArgs a{};
        a.n_lanes = n_requests;
        a.req = d_req.p; a.craft = craft ? d_craft.p : nullptr;
        a.slabs = knot_slabs(b);
        a.ev = event_args(b);
        if (!b->events) a.ev.max_tr = a.ev.max_ap = 0;
        a.seg_off = b->seg_off.p; a.segs = b->segs.p;
        a.ranges = d_ranges.p;
        std::vector<long long> lane_first(nr + 1, 0), first(nr + 1, 0);
        {
            PinnedStage stage(sizeof(int) * nr);        // the counts: 4 bytes per request, the call's one small synchronisation
            if (stage.status()) return stage.status();
            StreamIdleOnExit idle(s);
            static_assert(sizeof(long long) == sizeof(int64_t), "craft index type");
            if ((st = lanes.upload(s))) return st;
            EPH_HIP(hipMemcpyAsync(d_req.p, requests, sizeof(eph_marker_request) * nr, hipMemcpyHostToDevice, s));
            if (craft) EPH_HIP(hipMemcpyAsync(d_craft.p, craft, sizeof(int64_t) * nr, hipMemcpyHostToDevice, s));
            a.lane_item = lanes.d_item.p; a.lane_col = lanes.d_col.p;
            a.count = static_cast<int *>(stage.dev());
            if ((st = count_trace.kernel_begin())) return st;
            EPH_LAUNCH("k_craft_markers_count", k_craft_markers_count, dim3((unsigned)((nr + 63) / 64)), dim3(64), s, a);
            if ((st = count_trace.kernel_end())) return st;
            EPH_HIP(hipStreamSynchronize(s));
            idle.disarm();
            count_trace.copy_begin();
            const int *counts = static_cast<const int *>(stage.host());
            for (size_t l = 0; l < nr; ++l) {
                const long long cnt = std::max(counts[l], 0);
                lane_first[l + 1] = lane_first[l] + cnt;
                first[(size_t)lanes.item[l] + 1] = cnt;
            }
            for (size_t r = 0; r < nr; ++r) first[r + 1] += first[r];
            if ((st = count_trace.copy_end())) return st;
        }
        const size_t total = (size_t)first[nr];
        for (size_t r = 0; r <= nr; ++r) out_first[r] = (int64_t)first[r];
        if ((int64_t)total > marker_capacity) return EPH_ERR_BAD_ARGUMENT;
        long long passes = 0;
        if (total) {
            const size_t per_pass = std::min<size_t>(total, ((size_t)256 << 20) / sizeof(eph_plot_marker));
            DevBuf<eph_plot_marker> d_out;
            if ((st = d_out.alloc(per_pass))) return st;
            PinnedStage stage(sizeof(eph_plot_marker) * per_pass);
            if (stage.status()) return stage.status();
            StreamIdleOnExit idle(s);
            EPH_HIP(hipMemcpyAsync(d_first.p, lane_first.data(), sizeof(long long) * (nr + 1), hipMemcpyHostToDevice, s));
            a.count = nullptr; a.lane_first = d_first.p; a.out = d_out.p;
            const eph_plot_marker *staged = static_cast<const eph_plot_marker *>(stage.host());
            size_t lane = 0;                            // the lane that holds marker m0
            for (size_t m0 = 0; m0 < total; m0 += per_pass, ++passes) {
                const size_t m1 = std::min(total, m0 + per_pass);
                a.m0 = (long long)m0; a.m1 = (long long)m1;
                if ((st = trace.kernel_begin())) return st;
                EPH_LAUNCH("k_craft_markers_fill", k_craft_markers_fill, dim3((unsigned)((m1 - m0 + 63) / 64)), dim3(64), s, a);
                if ((st = trace.kernel_end())) return st;
                EPH_HIP(hipMemcpyAsync(stage.host(), d_out.p, sizeof(eph_plot_marker) * (m1 - m0), hipMemcpyDeviceToHost, s));
                EPH_HIP(hipStreamSynchronize(s));
                trace.copy_begin();
                while (lane < nr && (size_t)lane_first[lane + 1] <= m0) ++lane;
                for (size_t l = lane; l < nr && (size_t)lane_first[l] < m1; ++l) {     // each request's run to its place
                    const size_t from = std::max((size_t)lane_first[l], m0), to = std::min((size_t)lane_first[l + 1], m1);
                    if (from >= to) continue;
                    std::memcpy(out_markers + first[(size_t)lanes.item[l]] + (from - (size_t)lane_first[l]), staged + (from - m0),
                                sizeof(eph_plot_marker) * (to - from));
                }
                if ((st = trace.copy_end())) return st;
            }
            idle.disarm();
        }
        count_trace.report("craft_markers_count", "requests", (long long)n_requests, "markers", (long long)total, 1);
        trace.report("craft_markers_fill", "requests", (long long)n_requests, "markers", (long long)total, passes);
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
