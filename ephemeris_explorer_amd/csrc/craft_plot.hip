// craft_plot.hip -- the adaptive plot sampler on the knot slabs of a spacecraft batch (eph_craft_batch_plot_points): what
// eph_plot_points computes for a ship's knots, with the knots read where the sweep left them. Reads the batch; changes nothing in it.
//
// Mirrors compute_plot_points_parallel and PlotPoints::new (ephemeris_explorer/src/ui/world/plot.rs) over a CubicHermiteSpline
// relative to a body, through trajectory_eval.h, which carries the reference's line numbers.
// All of it is plot_sample of trajectory_eval.h, the sampler k_plot_points (evaluators.hip) runs too; this unit adds where the
// knots live (one column of the slabs) and where the points go.
//
// The way out: a lane stores point k at [k][lane] of a device block, so the lanes of a wave that are in step write neighbouring
// words; k_craft_plot_rows_out then copies the USED part of every row (k < count) into the pinned staging buffer as [lane][k], and
// the host moves each row to its plot's place in the caller's arrays. Entries at or beyond out_count[p] are never written. Storing
// rows [lane][k] from the sampler itself and copying whole rows was measured and dropped (profiles/craft_plot.md).
#include <algorithm>
#include <cstring>

#include "craft_batch.h"

namespace eph {

struct CraftPlotArgs {
    long long n_lanes;              // plots of this pass
    const long long *lane_plot;     // lane -> plot (the caller's index); lanes are ordered by slab column
    const int *lane_col;            // lane -> slab column of the plot's craft
    KnotSlabs slabs;
    BodyTable table;
    const eph_plot_request *req;    // [plot]
    eph_plot_view view;
    long long capacity;
    double *out_t;                  // [k][lane]
    float *out_xyz;                 // [k][3][lane]
    long long *out_count;           // [lane]
    int *out_status;
    double *out_failed_at;
};
struct ColumnSource {         // one craft's column of the knot slabs
    KnotColumn knots;
    __device__ __forceinline__ void bounds(double &start, double &end, long long &segs) const { hermite_bounds(knots, start, end, segs); }
    __device__ __forceinline__ bool state_vector(double t, V3 &p, V3 &v) const { return hermite_state_vector(knots, t, p, v); }
};
struct LaneSink {             // one lane's column of the results, [k][lane], and its three scalars
    long long nl;                   // lanes = the stride of a row
    double *t;
    float *xyz;
    long long *n;
    int *st;
    double *fail;
    __device__ __forceinline__ void push(long long k, double at, V3 q) const {
        t[k * nl] = at;
        xyz[(3 * k) * nl] = (float)q.x; xyz[(3 * k + 1) * nl] = (float)q.y; xyz[(3 * k + 2) * nl] = (float)q.z;
    }
    __device__ __forceinline__ void count(long long np) const { *n = np; }
    __device__ __forceinline__ void status(int s) const { *st = s; }
    __device__ __forceinline__ void failed_at(double at) const { *fail = at; }
};

// One lane per plot, plot_sample's sequential adaptive loop (trajectory_eval.h). The lanes of a pass are ordered by slab column (the
// host sorts them): craft that were dealt to neighbouring columns have similar time scales, so a wave's lanes ask for similar knot
// indices at similar epochs -- few cache lines per load -- and take similar numbers of points. 124 VGPRs (128 allocated), no
// scratch, 4 waves per SIMD.
__global__ void __launch_bounds__(64) k_craft_plot_points(const CraftPlotArgs a) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= a.n_lanes) return;
    const eph_plot_request rq = a.req[a.lane_plot[lane]];
    const ColumnSource src = {a.slabs.column(a.lane_col[lane])};
    LaneSink sink = {a.n_lanes, a.out_t + lane, a.out_xyz + lane, a.out_count + lane, a.out_status + lane, a.out_failed_at + lane};
    plot_sample(a.table, a.view, rq, src, sink);
}

// One pass of results from [k][lane] on the device to [lane][k] in the pinned staging buffer, one wave per lane's row: gathered
// reads of device memory (a line holds the same k of eight neighbouring lanes, whose waves are neighbours too), every store to host
// memory coalesced, and only the used part of a row travels.
__global__ void __launch_bounds__(64) k_craft_plot_rows_out(long long n_lanes, long long capacity, const double *__restrict__ t,
                                                            const float *__restrict__ xyz, const long long *__restrict__ count,
                                                            const int *__restrict__ status, const double *__restrict__ failed_at,
                                                            double *__restrict__ out_t, float *__restrict__ out_xyz,
                                                            long long *__restrict__ out_count, int *__restrict__ out_status,
                                                            double *__restrict__ out_failed_at) {
    const long long lane = blockIdx.x;
    if (lane >= n_lanes) return;
    const long long cnt = min(max(count[lane], 0LL), capacity);
    if (threadIdx.x == 0) {
        out_count[lane] = cnt;
        out_status[lane] = status[lane];
        out_failed_at[lane] = failed_at[lane];
    }
    for (long long k = threadIdx.x; k < cnt; k += blockDim.x) out_t[lane * capacity + k] = t[k * n_lanes + lane];
    for (long long j = threadIdx.x; j < 3 * cnt; j += blockDim.x) out_xyz[lane * capacity * 3 + j] = xyz[j * n_lanes + lane];
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_craft_batch_plot_points(eph_craft_batch *b, const eph_plot_view *view, int64_t n_plots,
                                    const eph_plot_request *requests, const int64_t *craft, int64_t capacity,
                                    double *out_t, float *out_xyz, int64_t *out_count, int32_t *out_status,
                                    double *out_failed_at) {
    EPH_GUARD_BEGIN
        if (!b || !view || n_plots < 0 || capacity < 0 ||
            (n_plots > 0 && (!requests || !out_count || !out_status || !out_failed_at)) ||
            (n_plots > 0 && capacity > 0 && (!out_t || !out_xyz)))
            return EPH_ERR_BAD_ARGUMENT;
        bool any_reference = false;
        for (int64_t p = 0; p < n_plots; ++p) {
            const eph_plot_request &r = requests[p];
            if (r.source_body != -1 || r.knot_first != 0 || r.knot_count != 0 || r.reference_body < -1 ||
                r.reference_body >= b->eph->n_bodies || r.max_points < 0 || r.max_points > capacity || r.bound < 0 || r.bound > 2)
                return EPH_ERR_BAD_ARGUMENT;
            any_reference = any_reference || r.reference_body >= 0;
        }
        if (n_plots == 0 || b->n == 0) return EPH_OK;
        const size_t np_all = (size_t)n_plots, cap = (size_t)capacity;
        LaneMap lanes;                                  // lanes in slab-column order
        int st;
        if ((st = lanes.sort(b, np_all, craft))) return st;
        const auto table_lock = table_lock_if(b->eph, any_reference);
        EPH_HIP(hipSetDevice(b->device));
        PassTrace trace("EPH_TRACE_CRAFT_PLOT", b);     // the call's kernel time and host copy time (scripts/craft_plot_timing.py)
        // passes over plots (in lane order): at most 256 MB of results each (one plot at least), through one device block [k][lane]
        // and the pinned staging buffer [lane][k]
        const size_t plot_bytes = cap * (sizeof(double) + 3 * sizeof(float)) + sizeof(double) + sizeof(int64_t) + sizeof(int32_t);
        const size_t per_pass = std::min<size_t>(np_all, std::max<size_t>(1, ((size_t)256 << 20) / plot_bytes));
        DevBuf<eph_plot_request> d_req;
        DevBuf<long long> d_cnt;
        DevBuf<int> d_st;
        DevBuf<double> d_t, d_fail;
        DevBuf<float> d_xyz;
        if ((st = d_req.alloc(np_all)) || (st = d_t.alloc(per_pass * cap)) || (st = d_xyz.alloc(3 * per_pass * cap)) ||
            (st = d_cnt.alloc(per_pass)) || (st = d_st.alloc(per_pass)) || (st = d_fail.alloc(per_pass)))
            return st;
        PinnedStage stage(per_pass * plot_bytes);
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(b->stream);
        hipStream_t s = b->stream;
        EPH_HIP(hipMemcpyAsync(d_req.p, requests, sizeof(eph_plot_request) * np_all, hipMemcpyHostToDevice, s));
        if ((st = lanes.upload(s))) return st;
        CraftPlotArgs a{};
        a.slabs = knot_slabs(b);
        a.table = body_table(b->eph);
        a.req = d_req.p; a.view = *view; a.capacity = capacity;
        a.out_t = d_t.p; a.out_xyz = d_xyz.p; a.out_count = d_cnt.p; a.out_status = d_st.p; a.out_failed_at = d_fail.p;
        // the staging buffer: t[lane][cap] | failed_at[lane] | count[lane] | xyz[lane][cap][3] | status[lane]
        static_assert(sizeof(long long) == sizeof(int64_t), "count type");
        double *stage_t = static_cast<double *>(stage.dev());
        double *stage_fail = stage_t + per_pass * cap;
        long long *stage_cnt = reinterpret_cast<long long *>(stage_fail + per_pass);
        float *stage_xyz = reinterpret_cast<float *>(stage_cnt + per_pass);
        int *stage_st = reinterpret_cast<int *>(stage_xyz + 3 * per_pass * cap);
        const double *host_t = stage.host_of(stage_t), *host_fail = stage.host_of(stage_fail);
        const long long *host_cnt = stage.host_of(stage_cnt);
        const float *host_xyz = stage.host_of(stage_xyz);
        const int *host_st = stage.host_of(stage_st);
        for (size_t l0 = 0; l0 < np_all; l0 += per_pass) {
            const size_t nl = std::min(per_pass, np_all - l0);
            a.n_lanes = (long long)nl;
            a.lane_plot = lanes.d_item.p + l0;
            a.lane_col = lanes.d_col.p + l0;
            if ((st = trace.kernel_begin())) return st;
            EPH_LAUNCH("k_craft_plot_points", k_craft_plot_points, dim3((unsigned)((nl + 63) / 64)), dim3(64), s, a);
            if ((st = trace.kernel_end())) return st;
            EPH_LAUNCH("k_craft_plot_rows_out", k_craft_plot_rows_out, dim3((unsigned)nl), dim3(64), s, (long long)nl, (long long)capacity,
                       (const double *)d_t.p, (const float *)d_xyz.p, (const long long *)d_cnt.p, (const int *)d_st.p,
                       (const double *)d_fail.p, stage_t, stage_xyz, stage_cnt, stage_st, stage_fail);
            EPH_HIP(hipStreamSynchronize(s));
            trace.copy_begin();
            for (size_t l = 0; l < nl; ++l) {
                const size_t p = (size_t)lanes.item[l0 + l];
                const size_t cnt = (size_t)std::min<long long>(std::max<long long>(host_cnt[l], 0), (long long)cap);
                out_count[p] = (int64_t)cnt;
                out_status[p] = host_st[l];
                out_failed_at[p] = host_fail[l];
                if (cnt) {
                    std::memcpy(out_t + p * cap, host_t + l * cap, sizeof(double) * cnt);
                    std::memcpy(out_xyz + p * cap * 3, host_xyz + l * cap * 3, sizeof(float) * 3 * cnt);
                }
            }
            if ((st = trace.copy_end())) return st;
        }
        idle.disarm();
        trace.report("craft_plot", "plots", (long long)n_plots, "capacity", (long long)capacity,
                     (long long)((np_all + per_pass - 1) / per_pass));
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
