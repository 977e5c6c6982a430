// craft_batch.h -- struct eph_craft_batch (craft.hip owns it) and what the units that read or restart a batch on the device share
// (craft_events.hip, craft_eval.hip, craft_plot.hip, craft_separation.hip, craft_restart.hip): the view of the knot slabs a kernel
// takes, the request-to-lane map, the pass timing of the EPH_TRACE_* variables, and the calls that cross between the units.
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
