// craft_separation.hip -- the closest-separation search of target plotting on the knot slabs of a spacecraft batch
// (eph_craft_batch_closest_separation): what eph_closest_separation computes for a ship's knots against a body of the live table or
// against another ship of the same batch, with the knots read where the sweep left them. Reads the batch; changes nothing in it.
//
// Mirrors setup_target_plotting (ephemeris_explorer/src/analysis.rs:308-371) over RelativeTrajectory::closest_separation_between,
// through trajectory_eval.h, which carries the reference's line numbers. All of it is closest_separation of trajectory_eval.h, the
// search k_closest_separation (evaluators.hip) runs too; this unit adds where the knots live (one column of the slabs per craft) and
// where the six scalars of a result go.
#include <algorithm>
#include <cstring>
#include <vector>

#include "craft_batch.h"

namespace eph {

struct SeparationRow {        // one request's result on its way out
    double time, distance, failed_at;
    int iterations, status, found, pad;
};
struct CraftSeparationArgs {
    long long n_lanes;              // requests
    const long long *lane_req;      // lane -> request (the caller's index); lanes are ordered by the source's slab column
    const int *lane_col;            // lane -> slab column of the source craft
    const int *lane_target_col;     // lane -> slab column of the target craft, -1: the target is the request's body
    KnotSlabs slabs;
    BodyTable table;
    const eph_separation_request *req;   // [request]
    SeparationRow *out;             // [lane]
};

// One lane per request, closest_separation's sequential ternary search (trajectory_eval.h). Lanes are ordered by the source's slab
// column (the host sorts them), as k_craft_plot_points' are: neighbouring columns hold craft of similar time scales, so a wave's lanes
// ask for similar knot indices at similar epochs.
__global__ void __launch_bounds__(64) k_craft_separation(const CraftSeparationArgs a) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= a.n_lanes) return;
    const eph_separation_request rq = a.req[a.lane_req[lane]];
    const long long tcol = a.lane_target_col[lane];
    const SeparationTrajectory<KnotColumn> src = {a.table, -1, a.slabs.column(a.lane_col[lane])};
    // a body target never reads its knots: the source's column stands in
    const SeparationTrajectory<KnotColumn> tgt = {a.table, tcol >= 0 ? -1 : rq.target_body,
                                                  a.slabs.column(tcol >= 0 ? tcol : a.lane_col[lane])};
    const Separation r = closest_separation(src, tgt, rq.left, rq.right, rq.precision, rq.max_iterations, rq.metric);
    a.out[lane] = {r.time, r.distance, r.failed_at, r.iterations, r.status, r.found, 0};
}

// The rows from device memory into the pinned staging buffer, still in lane order: the host moves each to its request's place.
__global__ void __launch_bounds__(256) k_craft_separation_rows_out(long long n_lanes, const SeparationRow *__restrict__ rows,
                                                                   SeparationRow *__restrict__ out) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane < n_lanes) out[lane] = rows[lane];
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_closest_separation(eph_craft_batch *b, int64_t n_requests, const eph_separation_request *requests,
                                           const int64_t *craft, const int64_t *target_craft,
                                           uint8_t *out_found, double *out_time, double *out_distance,
                                           int32_t *out_iterations, int32_t *out_status, double *out_failed_at) {
    EPH_GUARD_BEGIN
        if (!b || n_requests < 0 ||
            (n_requests > 0 && (!requests || !out_found || !out_time || !out_distance || !out_iterations || !out_status || !out_failed_at)))
            return EPH_ERR_BAD_ARGUMENT;
        bool any_body = false;
        for (int64_t p = 0; p < n_requests; ++p) {
            const eph_separation_request &r = requests[p];
            const bool by_craft = target_craft && target_craft[p] >= 0;
            if (r.source_body != -1 || r.source_knot_first != 0 || r.source_knot_count != 0 || r.target_knot_first != 0 ||
                r.target_knot_count != 0 || r.target_body < -1 || r.target_body >= b->eph->n_bodies ||
                by_craft == (r.target_body >= 0) || !separation_request_ok(r))
                return EPH_ERR_BAD_ARGUMENT;
            any_body = any_body || r.target_body >= 0;
        }
        if (n_requests == 0 || b->n == 0) return EPH_OK;
        const size_t np = (size_t)n_requests;
        LaneMap lanes;                                  // lanes in the order of the source's slab column
        int st;
        if ((st = lanes.sort(b, np, craft))) return st;
        for (int64_t p = 0; target_craft && p < n_requests; ++p)
            if (target_craft[p] >= b->n) return EPH_ERR_BAD_ARGUMENT;
        const bool dealt = !b->h_slot.empty();
        std::vector<int> lane_target_col(np);
        for (size_t l = 0; l < np; ++l) {
            const int64_t t = target_craft ? target_craft[lanes.item[l]] : -1;
            lane_target_col[l] = t < 0 ? -1 : (dealt ? b->h_slot[(size_t)t] : (int)t);
        }
        const auto table_lock = table_lock_if(b->eph, any_body);
        EPH_HIP(hipSetDevice(b->device));
        DevBuf<eph_separation_request> d_req;
        DevBuf<int> d_lane_target_col;
        DevBuf<SeparationRow> d_rows;
        if ((st = d_req.alloc(np)) || (st = d_lane_target_col.alloc(np)) || (st = d_rows.alloc(np))) return st;
        PinnedStage stage(np * sizeof(SeparationRow));
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(b->stream);
        hipStream_t s = b->stream;
        EPH_HIP(hipMemcpyAsync(d_req.p, requests, sizeof(eph_separation_request) * np, hipMemcpyHostToDevice, s));
        if ((st = lanes.upload(s))) return st;
        EPH_HIP(hipMemcpyAsync(d_lane_target_col.p, lane_target_col.data(), sizeof(int) * np, hipMemcpyHostToDevice, s));
        CraftSeparationArgs a{};
        a.n_lanes = n_requests; a.lane_req = lanes.d_item.p; a.lane_col = lanes.d_col.p; a.lane_target_col = d_lane_target_col.p;
        a.slabs = knot_slabs(b);
        a.table = body_table(b->eph);
        a.req = d_req.p; a.out = d_rows.p;
        EPH_LAUNCH("k_craft_separation", k_craft_separation, dim3((unsigned)((np + 63) / 64)), dim3(64), s, a);
        EPH_LAUNCH("k_craft_separation_rows_out", k_craft_separation_rows_out, dim3((unsigned)((np + 255) / 256)), dim3(256), s,
                   (long long)np, (const SeparationRow *)d_rows.p, static_cast<SeparationRow *>(stage.dev()));
        EPH_HIP(hipStreamSynchronize(s));
        idle.disarm();
        const SeparationRow *rows = static_cast<const SeparationRow *>(stage.host());
        for (size_t l = 0; l < np; ++l) {
            const size_t p = (size_t)lanes.item[l];
            out_found[p] = (uint8_t)rows[l].found;
            out_time[p] = rows[l].time;
            out_distance[p] = rows[l].distance;
            out_iterations[p] = rows[l].iterations;
            out_status[p] = rows[l].status;
            out_failed_at[p] = rows[l].failed_at;
        }
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
