// craft_batch.h -- struct eph_craft_batch (craft.hip owns it) and what the units that build, read or restart a batch share (craft_events,
// craft_eval, craft_plot, craft_markers, craft_separation, craft_restart, craft_gather .hip): the statement of its device buffers with the
// walks built on it, the knot slabs as a kernel takes them, the request-to-lane map, the EPH_TRACE_* pass timing, the calls between units.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ephemeris_table.h"

struct eph_craft_batch {
    int pv = 0;                               // evaluation order of the point-mass term this batch was created under
    const eph_ephemeris *eph = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    long long n = 0;
    int max_knots = 0;
    eph::ErkCoeffs rk{};
    eph_adaptive_params params{};
    eph::DevBuf<double> time, y, next_h, klast, kfirst, last_knot, knot_t, knot_y; // klast / kfirst: the FSAL pairs' k[S-1] / k[0] between calls
    eph::DevBuf<unsigned> n_attempts, rk_i, steps;
    eph::DevBuf<int> cur_seg, status, nknots;
    eph::DevBuf<long long> seg_off;
    eph::DevBuf<eph::SegmentDev> segs;
    std::vector<long long> h_seg_off;         // host mirror of seg_off / segs (eph_craft_batch_restart rebuilds the CSR from it)
    std::vector<eph::SegmentDev> h_segs;
    eph::DevBuf<double> t_start;              // creation epoch per craft: the trajectory start of the restart rule (knot 0 moves on a drain)
    eph::DevBuf<eph::ErkCoeffs> rk_dev;
    eph::DevBuf<eph_craft_record> summary;    // eph_craft_batch_summary's device-side records (a clone's: on first use)
    eph::DevBuf<unsigned long long> queue;    // k_craft_queue's work queue (one counter)
    bool heterogeneous = false;               // the craft's dynamical time scales differ widely (craft_time_scales): queue form
    eph::DevBuf<eph::BodyEntry> bodies_ordered; // eph_craft_batch_set_body_order: the ephemeris's table permuted (empty: table order),
    eph::DevBuf<int> body_order_dev;          //   re-gathered from the live table before every sweep
    std::vector<int32_t> body_order;
    bool retry = false;                       // eph_craft_batch_retry_failed: the next sweep steps the craft whose last step failed
    eph::DevBuf<int> perm, slot_of;           // heterogeneous batches: lane / queue position -> craft by dynamical time, and back
    std::vector<int> h_slot;                  //   (craft_sort); the knot slabs' columns are lane positions
    // SpacecraftSolout events (optional)
    bool events = false;
    int max_tr = 0, max_ap = 0;
    eph::DevBuf<double> soi, tr_time, ap_time, ap_dist;
    eph::DevBuf<int> ev_seg, ntr, nap, ev_status, tr_body, ap_body, ap_kind;
    double kernel_ms = 0;
    ~eph_craft_batch() {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
            (void)hipStreamDestroy(stream);
        }
    }
};

namespace eph {
// ---- The batch's device buffers, stated once ------------------------------------------------------------------------------------
// for_each_buffer names every DevBuf member of eph_craft_batch with its shape; allocation and eph_craft_batch_clone are walks over it. A NEW
// BUFFER IS ADDED TO THE STRUCT AND TO THAT LIST AND NOWHERE ELSE: beyond them a name appears only where a kernel argument block is filled,
// where a reader copies the buffer out and where its contents are initialised.
enum class BufGroup { craft, timeline, events, deal, body_order, single, scratch };
// rows x one element per: craft, craft and knot / transition / apsis (the slabs, [depth][rows][craft]), craft + 1, segment, body, lane, batch
enum class BufExtent { craft, knots, transitions, apsides, craft_plus_one, segments, bodies, lanes, one };
enum class BufClone { copy, fresh, first_use };                              // copied | allocated, contents not carried | left empty
struct BufShape { BufGroup group; BufExtent extent; int rows = 1; BufClone clone = BufClone::copy; };
struct BatchDims { long long n; int max_knots; size_t n_segs; int max_tr, max_ap, n_bodies; };
inline size_t buffer_count(const BufShape &s, const BatchDims &d) {
    const size_t n = (size_t)d.n, per_craft = (size_t)s.rows * std::max<size_t>(n, 1);
    const size_t count[] = {per_craft, per_craft * std::max(d.max_knots, 1), per_craft * std::max(d.max_tr, 1), per_craft * std::max(d.max_ap, 1), n + 1,
                            std::max<size_t>(d.n_segs, 1), (size_t)std::max(d.n_bodies, 1), (n + 3) & ~(size_t)3, 1};   // in BufExtent's order
    return count[(int)s.extent];                                         // (lanes: whole 16-byte granules, craft_sort's k_copy16)
}
template <typename F>            // f(pointer to the member, its shape) for every buffer, until one returns a status other than EPH_OK: that status
int for_each_buffer(F &&f) {
    using B = eph_craft_batch; using G = BufGroup; using E = BufExtent;
    constexpr BufShape craft1{G::craft, E::craft}, craft6{G::craft, E::craft, 6}, knots1{G::craft, E::knots}, knots6{G::craft, E::knots, 6};
    constexpr BufShape offsets{G::timeline, E::craft_plus_one}, segments{G::timeline, E::segments}, deal{G::deal, E::lanes};
    constexpr BufShape radii{G::events, E::bodies}, event1{G::events, E::craft}, tr{G::events, E::transitions}, ap{G::events, E::apsides};
    constexpr BufShape order{G::body_order, E::bodies}, single{G::single, E::one};
    constexpr BufShape counter{G::single, E::one, 1, BufClone::fresh};            // queue: reset before every sweep that uses it
    constexpr BufShape scratch{G::scratch, E::craft, 1, BufClone::first_use};     // summary: never copied
    int st;
    (void)((st = f(&B::time, craft1)) || (st = f(&B::y, craft6)) || (st = f(&B::next_h, craft1)) || (st = f(&B::klast, craft6)) || (st = f(&B::kfirst, craft6)) ||
        (st = f(&B::last_knot, craft1)) || (st = f(&B::t_start, craft1)) || (st = f(&B::n_attempts, craft1)) || (st = f(&B::rk_i, craft1)) ||
        (st = f(&B::steps, craft1)) || (st = f(&B::cur_seg, craft1)) || (st = f(&B::status, craft1)) || (st = f(&B::nknots, craft1)) ||
        (st = f(&B::knot_t, knots1)) || (st = f(&B::knot_y, knots6)) || (st = f(&B::seg_off, offsets)) || (st = f(&B::segs, segments)) ||
        (st = f(&B::soi, radii)) || (st = f(&B::ev_seg, event1)) || (st = f(&B::ntr, event1)) || (st = f(&B::nap, event1)) || (st = f(&B::ev_status, event1)) ||
        (st = f(&B::tr_time, tr)) || (st = f(&B::tr_body, tr)) || (st = f(&B::ap_time, ap)) || (st = f(&B::ap_dist, ap)) || (st = f(&B::ap_body, ap)) ||
        (st = f(&B::ap_kind, ap)) || (st = f(&B::perm, deal)) || (st = f(&B::slot_of, deal)) || (st = f(&B::bodies_ordered, order)) ||
        (st = f(&B::body_order_dev, order)) || (st = f(&B::rk_dev, single)) || (st = f(&B::queue, counter)) || (st = f(&B::summary, scratch)));
    return st;
}
template <typename Keep>                                               // the buffers of the groups `keep` says yes to, at d's element counts
int alloc_buffers(eph_craft_batch *b, const BatchDims &d, Keep &&keep) {
    return for_each_buffer([&](auto member, const BufShape &s) { return keep(s.group) ? (b->*member).alloc(buffer_count(s, d)) : EPH_OK; });
}
// what create and gather allocate before the contents arrive: per-craft state, knot slabs, the timeline CSR of n_segs segments, rk_dev,
// queue and summary (here, not at the first eph_craft_batch_summary: keeps hipMalloc out of a sweep)
inline int alloc_state(eph_craft_batch *b, long long n, int max_knots, size_t n_segs) {
    const auto mine = [](BufGroup g) { return g != BufGroup::events && g != BufGroup::deal && g != BufGroup::body_order; };
    return alloc_buffers(b, BatchDims{n, max_knots, n_segs, 0, 0, 0}, mine);
}
// what enable_events and gather allocate: the event state, the event slabs and the sphere radii of b
inline int alloc_events(eph_craft_batch *b, int max_tr, int max_ap) {
    return alloc_buffers(b, BatchDims{b->n, 0, 0, max_tr, max_ap, b->eph->n_bodies}, [](BufGroup g) { return g == BufGroup::events; });
}
// eph_craft_batch_clone's walk: every buffer `src` has, by src's count, on stream `s`; the caller synchronises
inline int copy_buffers(const eph_craft_batch *src, eph_craft_batch *dst, hipStream_t s) {
    return for_each_buffer([&](auto m, const BufShape &sh) {
        return sh.clone == BufClone::copy ? copy_buf(src->*m, dst->*m, s) : sh.clone == BufClone::fresh ? (dst->*m).alloc((src->*m).count) : (int)EPH_OK;
    });
}
// craft.hip: a new batch of n craft with its stream and two events on model's device (which is current) and model's settings -- pv, eph,
// device, rk, params, events, max_tr, max_ap, retry, body_order, heterogeneous -- and no buffer
int craft_batch_shell(const eph_craft_batch &model, long long n, int max_knots, std::unique_ptr<eph_craft_batch> &out);

bool craft_wave_form(long long n_craft);                  // craft.hip: one wave per craft (few spacecraft) or one thread
int craft_events_search(eph_craft_batch *b, hipStream_t s);   // craft_events.hip: the event search on the steps a sweep just took
// craft.hip: the creation rule's deal of a thread-per-craft batch to the lanes from its current time and state (perm, slot_of, h_slot;
// nothing when the gate -- EPH_CRAFT_SORT, n >= 128, not the wave form -- says no deal). knot0_to_lanes: creation's tail, knot 0
// (uploaded in craft order) moves to the lanes' columns; eph_craft_batch_gather moves whole columns itself. The caller holds the
// table's read lock and has the batch's device current; the batch's stream is idle on return.
int craft_sort(eph_craft_batch *b, bool knot0_to_lanes);
// craft.hip: Timeline::new (spacecraft.rs:129-152) of one craft's burns, appended to `segs` (create, restart, divergence time)
void timeline_new(long long nburns, const double *burn_start, const double *burn_end, const double *burn_acc, const int32_t *burn_ref,
                  std::vector<SegmentDev> &segs);
// craft.hip: a burn CSR over n craft, caller memory, checked before its first use -- offsets (non-negative start, never decreasing),
// the arrays present when a burn is (`from_zero`, creation's rule: whenever the CSR ends beyond 0), burn_ref = -1 or a body index for
// every craft that `which` keeps (null: all): any of them EPH_ERR_BAD_ARGUMENT.
int burn_csr_check(long long n, const int64_t *burn_offset, const double *burn_start, const double *burn_end, const double *burn_acc,
                   const int32_t *burn_ref, int n_bodies, const uint8_t *which, bool from_zero);
// craft.hip: on a checked CSR, EPH_ERR_UNSUPPORTED and its text for a kept burn in a frame built from the velocity (ERKN pairs)
int burn_erkn_check(long long n, const int64_t *burn_offset, const int32_t *burn_ref, const uint8_t *which);

// The knot slabs as a kernel reads them. The columns are lane positions (craft_sort): column() translates through `perm`.
struct KnotSlabs {
    long long n;                 // craft = columns of the slabs
    int max_knots;
    const int *nknots;           // [craft]
    const int *perm;             // slab column -> craft (null: identity)
    const double *knot_t;        // [k][column]
    const double *knot_y;        // [k][6][column]
    __device__ __forceinline__ long long craft_of(long long col) const { return perm ? perm[col] : col; }
    __device__ __forceinline__ KnotColumn column(long long col) const { return column(col, craft_of(col)); }
    // for k_craft_eval, which indexes its epochs by craft_of(col) too: through column(col) it loaded perm[col] twice (one more VMEM load)
    __device__ __forceinline__ KnotColumn column(long long col, long long craft) const {
        return KnotColumn{min(max(nknots[craft], 0), max_knots), n, knot_t + col, knot_y + col};
    }
};
inline KnotSlabs knot_slabs(const eph_craft_batch *b) {
    return {b->n, b->max_knots, b->nknots.p, b->h_slot.empty() ? nullptr : b->perm.p, b->knot_t.p, b->knot_y.p};
}
// Lanes in slab-column order for the units that run one lane per request over a craft's knot column (craft_plot.hip,
// craft_separation.hip): request p reads craft craft[p] (null: craft p); lane l serves request lane_item[l] and reads column
// lane_col[l]. A counting sort by column, stable in request order; an undealt batch asked craft by craft is in that order already.
inline void lanes_by_column(const eph_craft_batch *b, size_t n_items, const int64_t *craft, std::vector<long long> &lane_item,
                            std::vector<int> &lane_col) {
    const size_t n = (size_t)b->n;
    const bool dealt = !b->h_slot.empty();
    lane_item.resize(n_items);
    lane_col.resize(n_items);
    if (!dealt && !craft) {
        for (size_t p = 0; p < n_items; ++p) { lane_item[p] = (long long)p; lane_col[p] = (int)p; }
        return;
    }
    auto column = [&](size_t p) { const size_t c = craft ? (size_t)craft[p] : p; return dealt ? (size_t)b->h_slot[c] : c; };
    std::vector<size_t> first(n + 1, 0);
    for (size_t p = 0; p < n_items; ++p) first[column(p) + 1] += 1;
    for (size_t c = 0; c < n; ++c) first[c + 1] += first[c];
    for (size_t p = 0; p < n_items; ++p) {
        const size_t c = column(p), l = first[c]++;
        lane_item[l] = (long long)p; lane_col[l] = (int)c;
    }
}
// lanes_by_column of a call's requests, on the device as well
struct LaneMap {
    std::vector<long long> item;          // lane -> request
    std::vector<int> col;                 // lane -> slab column of the request's craft
    DevBuf<long long> d_item;
    DevBuf<int> d_col;
    // EPH_ERR_BAD_ARGUMENT: more requests than craft without `craft`, or a craft[p] outside the batch
    int sort(const eph_craft_batch *b, size_t n_items, const int64_t *craft) {
        if (!craft && (long long)n_items > b->n) return EPH_ERR_BAD_ARGUMENT;
        if (craft)
            for (size_t p = 0; p < n_items; ++p)
                if (craft[p] < 0 || craft[p] >= b->n) return EPH_ERR_BAD_ARGUMENT;
        lanes_by_column(b, n_items, craft, item, col);
        return EPH_OK;
    }
    int upload(hipStream_t s) {           // the batch's device is current
        int st;
        if ((st = d_item.alloc(item.size())) || (st = d_col.alloc(col.size()))) return st;
        EPH_HIP(hipMemcpyAsync(d_item.p, item.data(), sizeof(long long) * item.size(), hipMemcpyHostToDevice, s));
        EPH_HIP(hipMemcpyAsync(d_col.p, col.data(), sizeof(int) * col.size(), hipMemcpyHostToDevice, s));
        return EPH_OK;
    }
};
// EPH_TRACE_<UNIT>=1: the kernel time (between the batch's two events) and the host copy time of a call's passes, printed as the
// line scripts/<unit>_timing.py parses. With the variable unset no event is recorded and no clock is read.
struct PassTrace {
    bool on;
    const eph_craft_batch *b;
    double kernel_ms = 0.0, copy_ms = 0.0;
    std::chrono::steady_clock::time_point c0;
    PassTrace(const char *variable, const eph_craft_batch *batch) : b(batch) {
        const char *env = getenv(variable);
        on = env && atoi(env) != 0;
    }
    int kernel_begin() { if (on) EPH_HIP(hipEventRecord(b->ev0, b->stream)); return EPH_OK; }
    int kernel_end() { if (on) EPH_HIP(hipEventRecord(b->ev1, b->stream)); return EPH_OK; }
    void copy_begin() { if (on) c0 = std::chrono::steady_clock::now(); }     // after the stream's synchronisation
    int copy_end() {
        if (!on) return EPH_OK;
        float ms = 0.0f;
        EPH_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
        kernel_ms += ms;
        copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
        return EPH_OK;
    }
    void report(const char *unit, const char *what1, long long v1, const char *what2, long long v2, long long passes) const {
        if (on)
            fprintf(stderr, "%s: %s %lld %s %lld passes %lld kernel_ms %.4f host_copy_ms %.4f\n", unit, what1, v1, what2, v2, passes,
                    kernel_ms, copy_ms);
    }
};
}  // namespace eph
