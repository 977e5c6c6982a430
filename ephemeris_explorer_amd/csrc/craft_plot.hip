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
//
// eph_craft_batch_plot_segments puts setup_segment_plotting (ephemeris_explorer/src/analysis.rs:159-296) in front of the same sampler
// run: k_craft_plot_segments composes the records and the requests of a frame from the transition slabs and the timeline CSR, on the
// device, and plot_passes -- the pass loop both entry points share -- draws them.
#include <algorithm>
#include <climits>
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


struct CraftSegmentArgs {
    long long n_entries, n_craft;
    int n_bodies, max_tr;
    const eph_orbit_plot_config *cfg;   // [entry]
    const long long *craft;             // [entry], null: entry p is craft p
    const int *body_parent;             // [n_bodies]
    const int *ntr;                     // [craft]
    const double *tr_time;              // [k][craft]
    const int *tr_body;
    const long long *seg_off;           // the timeline CSR
    const SegmentDev *segs;
    int *count;                         // the count form: records per entry
    const long long *first;             // the fill form: [entries + 1] exclusive prefix sum of `count`
    eph_plot_segment *seg_out;          // [record]
    eph_plot_request *req_out;          // [record]
};

// setup_segment_plotting (analysis.rs:204-293) for one (craft, OrbitPlotConfig) entry per lane: the walk over the craft's column of
// the transition slab, the two lower-bound searches of Timeline::segments_between (ephemeris/src/propagators/spacecraft.rs:165-177)
// on its slice of the CSR, the kind. FILL = false counts the records (one integer per entry); FILL = true, run after the host's
// prefix sum, writes record first[p] + j and the eph_plot_request that draws it. A handful of records per entry and a few dozen
// bytes each: the lanes' work is uneven and the stores are scattered, and it is microseconds either way (profiles/craft_segments.md).
template <bool FILL>
__global__ void __launch_bounds__(64) k_craft_plot_segments(const CraftSegmentArgs a) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_entries) return;
    const eph_orbit_plot_config cfg = a.cfg[p];
    const long long c = a.craft ? a.craft[p] : p, n = a.n_craft;
    const int ntr = min(max(a.ntr[c], 0), a.max_tr);
    const SegmentDev *segs = a.segs + a.seg_off[c];
    const int nseg = (int)(a.seg_off[c + 1] - a.seg_off[c]);
    long long at = FILL ? a.first[p] : 0;
    const long long stop = FILL ? a.first[p + 1] : 0;        // (never written past: the entry's share of the arrays)
    for (int i = 0; i < ntr; ++i) {
        const double t_i = a.tr_time[(long long)i * n + c];
        const bool has_next = i + 1 < ntr, has_prev = i > 0;
        const double t_next = has_next ? a.tr_time[(long long)(i + 1) * n + c] : 0.0;
        if (t_i > cfg.end || (has_next && t_next < cfg.start)) continue;                        // :208-210
        const int b = a.tr_body[(long long)i * n + c];
        const int b_parent = b >= 0 && b < a.n_bodies ? a.body_parent[b] : -1;                  // :213-217 (the root: -1)
        const double start = t_i > cfg.start ? t_i : cfg.start;                                // :220 Ord::max(t_i, config.start)
        const double end = has_next ? (t_next <= cfg.end ? t_next : cfg.end) : cfg.end;        // :221 Ord::min
        int lo = 0, hi = nseg;                          // partition_point(seg.end <= start)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (segs[mid].end <= start) lo = mid + 1; else hi = mid;
        }
        const int k0 = lo;
        lo = 0; hi = nseg;                              // partition_point(seg.start < end)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (segs[mid].start < end) lo = mid + 1; else hi = mid;
        }
        const int k1 = lo;
        if (k0 >= k1) continue;                         // (k0 > k1: the reference's slice panics)
        const bool from = has_prev && b_parent >= 0 && a.tr_body[(long long)(i - 1) * n + c] == b_parent;   // :227-228
        const bool to = has_next && b_parent >= 0 && a.tr_body[(long long)(i + 1) * n + c] == b_parent;
        const int kind = from && to ? 2 : (from ? 0 : (to ? 1 : (has_prev || has_next ? 3 : 4)));
        const bool copy = kind == 2 && cfg.reference_body < 0;                                  // :254
        if (!FILL) {
            at += (long long)(k1 - k0) * (copy ? 2 : 1);
            continue;
        }
        for (int k = k0; k < k1; ++k) {
            const SegmentDev sg = segs[k];
            const double s0 = sg.start > start ? sg.start : start;                              // :230 Ord::max(seg.start, start)
            const double s1 = sg.end <= end ? sg.end : end;                                     // :231 Ord::min(seg.end, end)
            for (int o = 0; o < (copy ? 2 : 1) && at < stop; ++o) {
                const int reference = o ? b_parent : (cfg.reference_body >= 0 ? cfg.reference_body : b);
                a.seg_out[at] = eph_plot_segment{p, i, k, b, reference, kind, sg.is_burn ? 1 : 0, o, s0, s1};
                a.req_out[at] = eph_plot_request{-1, reference, 0, 0, s0, s1, cfg.bound, cfg.enabled, cfg.tan2_angular_resolution,
                                                 cfg.max_points_per_segment};
                at += 1;
            }
        }
    }
    if (!FILL) a.count[p] = (int)min(at, (long long)INT_MAX);
}


// The sampler run both entry points end in: the requests `d_req` (device memory, indexed by lanes.item) drawn on the knot slabs in
// passes over the lanes of at most 256 MB of results each (one plot at least), through one device block [k][lane] and the pinned
// staging buffer [lane][k]; row lanes.item[l] of the caller's five arrays is lane l's. The batch's device is current, the table
// lock (if a request names a body) is the caller's, and so is the report of `trace`. *passes: how many passes it took.
static int plot_passes(eph_craft_batch *b, const eph_plot_view &view, const eph_plot_request *d_req, LaneMap &lanes, int64_t capacity,
                       double *out_t, float *out_xyz, int64_t *out_count, int32_t *out_status, double *out_failed_at, PassTrace &trace,
                       long long *passes) {
    const size_t np_all = lanes.item.size(), cap = (size_t)capacity;
    int st;
    const size_t plot_bytes = cap * (sizeof(double) + 3 * sizeof(float)) + sizeof(double) + sizeof(int64_t) + sizeof(int32_t);
    const size_t per_pass = std::min<size_t>(np_all, std::max<size_t>(1, ((size_t)256 << 20) / plot_bytes));
    DevBuf<long long> d_cnt;
    DevBuf<int> d_st;
    DevBuf<double> d_t, d_fail;
    DevBuf<float> d_xyz;
    if ((st = d_t.alloc(per_pass * cap)) || (st = d_xyz.alloc(3 * per_pass * cap)) || (st = d_cnt.alloc(per_pass)) ||
        (st = d_st.alloc(per_pass)) || (st = d_fail.alloc(per_pass)))
        return st;
    PinnedStage stage(per_pass * plot_bytes);
    if (stage.status()) return stage.status();
    StreamIdleOnExit idle(b->stream);
    hipStream_t s = b->stream;
    if ((st = lanes.upload(s))) return st;
    CraftPlotArgs a{};
    a.slabs = knot_slabs(b);
    a.table = body_table(b->eph);
    a.req = d_req; a.view = view; a.capacity = capacity;
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
    *passes = (long long)((np_all + per_pass - 1) / per_pass);
    return EPH_OK;
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
        const size_t np_all = (size_t)n_plots;
        LaneMap lanes;                                  // lanes in slab-column order
        int st;
        if ((st = lanes.sort(b, np_all, craft))) return st;
        const auto table_lock = table_lock_if(b->eph, any_reference);
        EPH_HIP(hipSetDevice(b->device));
        PassTrace trace("EPH_TRACE_CRAFT_PLOT", b);     // the call's kernel time and host copy time (scripts/craft_plot_timing.py)
        DevBuf<eph_plot_request> d_req;
        if ((st = d_req.alloc(np_all))) return st;
        StreamIdleOnExit idle(b->stream);
        EPH_HIP(hipMemcpyAsync(d_req.p, requests, sizeof(eph_plot_request) * np_all, hipMemcpyHostToDevice, b->stream));
        long long passes = 0;
        if ((st = plot_passes(b, *view, d_req.p, lanes, capacity, out_t, out_xyz, out_count, out_status, out_failed_at, trace, &passes)))
            return st;
        idle.disarm();
        trace.report("craft_plot", "plots", (long long)n_plots, "capacity", (long long)capacity, passes);
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_craft_batch_plot_segments(eph_craft_batch *b, int64_t n_plots, const eph_orbit_plot_config *configs,
                                      const int64_t *craft, const int32_t *body_parent,
                                      int64_t segment_capacity, eph_plot_segment *out_segments, int64_t *out_first,
                                      const eph_plot_view *view, int64_t capacity, double *out_t, float *out_xyz,
                                      int64_t *out_count, int32_t *out_status, double *out_failed_at) {
    EPH_GUARD_BEGIN
        if (!b || !b->events || n_plots < 0 || segment_capacity < 0 || (segment_capacity > 0 && !out_segments) ||
            (n_plots > 0 && (!configs || !body_parent || !out_first)))
            return EPH_ERR_BAD_ARGUMENT;
        if (view && (capacity < 0 || (n_plots > 0 && (!out_count || !out_status || !out_failed_at)) ||
                     (n_plots > 0 && capacity > 0 && (!out_t || !out_xyz))))
            return EPH_ERR_BAD_ARGUMENT;
        const int nb = b->eph->n_bodies;
        for (int64_t p = 0; p < n_plots; ++p) {
            const eph_orbit_plot_config &c = configs[p];
            if (c.reference_body < -1 || c.reference_body >= nb || c.start != c.start || c.end != c.end || c.bound < 0 || c.bound > 2 ||
                c.max_points_per_segment < 0 || (view && c.max_points_per_segment > capacity))
                return EPH_ERR_BAD_ARGUMENT;
        }
        for (int q = 0; n_plots > 0 && q < nb; ++q)
            if (body_parent[q] < -1 || body_parent[q] >= nb || body_parent[q] == q) return EPH_ERR_BAD_ARGUMENT;
        const size_t ne = (size_t)n_plots;
        if (!craft && n_plots > b->n) return EPH_ERR_BAD_ARGUMENT;
        for (size_t p = 0; craft && p < ne; ++p)
            if (craft[p] < 0 || craft[p] >= b->n) return EPH_ERR_BAD_ARGUMENT;
        if (n_plots == 0 || b->n == 0) return EPH_OK;
        // a record's reference is always a body (the sphere's, its parent or the config's)
        const auto table_lock = table_lock_if(b->eph, view != nullptr);
        EPH_HIP(hipSetDevice(b->device));
        // kernel time and host time of the three steps (scripts/craft_segments_timing.py): the count with the host's scan, the fill
        // with the lane sort, the sampler with its row copies
        PassTrace count_trace("EPH_TRACE_CRAFT_SEGMENTS", b), fill_trace("EPH_TRACE_CRAFT_SEGMENTS", b),
            trace("EPH_TRACE_CRAFT_SEGMENTS", b);
        hipStream_t s = b->stream;
        int st;
        DevBuf<eph_orbit_plot_config> d_cfg;
        DevBuf<long long> d_craft, d_first;
        DevBuf<int> d_parent;
        if ((st = d_cfg.alloc(ne)) || (st = d_craft.alloc(craft ? ne : 0)) || (st = d_first.alloc(ne + 1)) || (st = d_parent.alloc((size_t)nb)))
            return st;
        CraftSegmentArgs a{};
        a.n_entries = n_plots; a.n_craft = b->n; a.n_bodies = nb; a.max_tr = b->max_tr;
        a.cfg = d_cfg.p; a.craft = craft ? d_craft.p : nullptr; a.body_parent = d_parent.p;
        a.ntr = b->ntr.p; a.tr_time = b->tr_time.p; a.tr_body = b->tr_body.p;
        a.seg_off = b->seg_off.p; a.segs = b->segs.p;
        const dim3 grid((unsigned)((ne + 63) / 64)), block(64);
        std::vector<long long> first(ne + 1, 0);
        {
            PinnedStage stage(sizeof(int) * ne);        // the counts: 4 bytes per entry, the call's one small synchronisation
            if (stage.status()) return stage.status();
            StreamIdleOnExit idle(s);
            static_assert(sizeof(long long) == sizeof(int64_t), "craft index type");
            EPH_HIP(hipMemcpyAsync(d_cfg.p, configs, sizeof(eph_orbit_plot_config) * ne, hipMemcpyHostToDevice, s));
            if (craft) EPH_HIP(hipMemcpyAsync(d_craft.p, craft, sizeof(int64_t) * ne, hipMemcpyHostToDevice, s));
            if (nb) EPH_HIP(hipMemcpyAsync(d_parent.p, body_parent, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, s));
            a.count = static_cast<int *>(stage.dev());
            if ((st = count_trace.kernel_begin())) return st;
            EPH_LAUNCH("k_craft_plot_segments<count>", k_craft_plot_segments<false>, grid, block, s, a);
            if ((st = count_trace.kernel_end())) return st;
            EPH_HIP(hipStreamSynchronize(s));
            idle.disarm();
            count_trace.copy_begin();
            const int *counts = static_cast<const int *>(stage.host());
            for (size_t p = 0; p < ne; ++p) first[p + 1] = first[p] + std::max(counts[p], 0);
            if ((st = count_trace.copy_end())) return st;
        }
        const size_t total = (size_t)first[ne];
        for (size_t p = 0; p <= ne; ++p) out_first[p] = (int64_t)first[p];
        if ((int64_t)total > segment_capacity) return EPH_ERR_BAD_ARGUMENT;
        long long passes = 0;
        if (total) {
            DevBuf<eph_plot_segment> d_seg;
            DevBuf<eph_plot_request> d_req;
            if ((st = d_seg.alloc(total)) || (st = d_req.alloc(total))) return st;
            PinnedStage stage(sizeof(eph_plot_segment) * total);
            if (stage.status()) return stage.status();
            StreamIdleOnExit idle(s);
            EPH_HIP(hipMemcpyAsync(d_first.p, first.data(), sizeof(long long) * (ne + 1), hipMemcpyHostToDevice, s));
            EPH_HIP(hipMemsetAsync(d_seg.p, 0, sizeof(eph_plot_segment) * total, s));     // (a record's padding bytes: zero, not leftovers)
            a.count = nullptr; a.first = d_first.p; a.seg_out = d_seg.p; a.req_out = d_req.p;
            if ((st = fill_trace.kernel_begin())) return st;
            EPH_LAUNCH("k_craft_plot_segments<fill>", k_craft_plot_segments<true>, grid, block, s, a);
            if ((st = fill_trace.kernel_end())) return st;
            EPH_HIP(hipMemcpyAsync(stage.host(), d_seg.p, sizeof(eph_plot_segment) * total, hipMemcpyDeviceToHost, s));
            if (fill_trace.on) EPH_HIP(hipStreamSynchronize(s));        // (the events are the batch's: read before the sampler records them)
            fill_trace.copy_begin();
            LaneMap lanes;                              // the host knows each record's craft from the scan: lanes in slab-column order
            if (view) {
                std::vector<int64_t> record_craft(total);
                for (size_t p = 0; p < ne; ++p)
                    std::fill(record_craft.begin() + first[p], record_craft.begin() + first[p + 1], craft ? craft[p] : (int64_t)p);
                if ((st = lanes.sort(b, total, record_craft.data()))) return st;
            }
            if ((st = fill_trace.copy_end())) return st;
            if (view) {
                if ((st = plot_passes(b, *view, d_req.p, lanes, capacity, out_t, out_xyz, out_count, out_status, out_failed_at, trace,
                                      &passes)))
                    return st;
            } else {
                EPH_HIP(hipStreamSynchronize(s));
            }
            idle.disarm();
            std::memcpy(out_segments, stage.host(), sizeof(eph_plot_segment) * total);
        }
        count_trace.report("craft_segments_count", "entries", (long long)n_plots, "records", (long long)total, 1);
        fill_trace.report("craft_segments_fill", "entries", (long long)n_plots, "records", (long long)total, total ? 1 : 0);
        trace.report("craft_segments_points", "records", (long long)total, "capacity", view ? (long long)capacity : 0, passes);
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
