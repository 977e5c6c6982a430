// craft_batch.h -- struct eph_craft_batch (craft.hip owns it) for craft_events.hip, whose entry points fill and read the batch's
// event slabs, and the two calls that cross between the two units.
#pragma once
#include <cstdint>
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
// craft.hip: Timeline::new (spacecraft.rs:129-152) of one craft's burns, appended to `segs` (create, restart, divergence time)
void timeline_new(long long nburns, const double *burn_start, const double *burn_end, const double *burn_acc, const int32_t *burn_ref,
                  std::vector<SegmentDev> &segs);
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
}  // namespace eph
