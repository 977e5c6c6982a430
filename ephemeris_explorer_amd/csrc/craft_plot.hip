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
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <shared_mutex>
#include <vector>

#include "craft_batch.h"
#include "trajectory_eval.h"

namespace eph {

struct CraftPlotArgs {
    long long n_lanes;              // plots of this pass
    const long long *lane_plot;     // lane -> plot (the caller's index); lanes are ordered by slab column
    const int *lane_col;            // lane -> slab column of the plot's craft
    long long n;                    // craft = columns of the slabs
    int max_knots;
    const int *nknots;              // [craft]
    const int *perm;                // slab column -> craft (null: identity)
    const double *knot_t;           // [k][column]
    const double *knot_y;           // [k][6][column]
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
    const long long col = a.lane_col[lane];
    const long long craft = a.perm ? a.perm[col] : col;
    const ColumnSource src = {KnotColumn{min(max(a.nknots[craft], 0), a.max_knots), a.n, a.knot_t + col, a.knot_y + col}};
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
    try {
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
        if (!craft && n_plots > b->n) return EPH_ERR_BAD_ARGUMENT;
        if (craft)
            for (int64_t p = 0; p < n_plots; ++p)
                if (craft[p] < 0 || craft[p] >= b->n) return EPH_ERR_BAD_ARGUMENT;
        const size_t np_all = (size_t)n_plots, cap = (size_t)capacity;
        // lanes in slab-column order (craft_batch.h)
        const bool dealt = !b->h_slot.empty();
        std::vector<long long> lane_plot;
        std::vector<int> lane_col;
        lanes_by_column(b, np_all, craft, lane_plot, lane_col);
        std::shared_lock<std::shared_mutex> table_lock(b->eph->mu, std::defer_lock);
        if (any_reference) table_lock.lock();
        EPH_HIP(hipSetDevice(b->device));
        // EPH_TRACE_CRAFT_PLOT=1 prints the call's kernel time and host copy time (scripts/craft_plot_timing.py)
        const char *env = getenv("EPH_TRACE_CRAFT_PLOT");
        const bool trace = env && atoi(env) != 0;
        // passes over plots (in lane order): at most 256 MB of results each (one plot at least), through one device block [k][lane]
        // and the pinned staging buffer [lane][k]
        const size_t plot_bytes = cap * (sizeof(double) + 3 * sizeof(float)) + sizeof(double) + sizeof(int64_t) + sizeof(int32_t);
        const size_t per_pass = std::min<size_t>(np_all, std::max<size_t>(1, ((size_t)256 << 20) / plot_bytes));
        DevBuf<eph_plot_request> d_req;
        DevBuf<long long> d_lane_plot, d_cnt;
        DevBuf<int> d_lane_col, d_st;
        DevBuf<double> d_t, d_fail;
        DevBuf<float> d_xyz;
        int st;
        if ((st = d_req.alloc(np_all)) || (st = d_lane_plot.alloc(np_all)) || (st = d_lane_col.alloc(np_all)) ||
            (st = d_t.alloc(per_pass * cap)) || (st = d_xyz.alloc(3 * per_pass * cap)) || (st = d_cnt.alloc(per_pass)) ||
            (st = d_st.alloc(per_pass)) || (st = d_fail.alloc(per_pass)))
            return st;
        PinnedStage stage(per_pass * plot_bytes);
        if (stage.status()) return stage.status();
        StreamIdleOnExit idle(b->stream);
        hipStream_t s = b->stream;
        hipError_t he;
        EPH_HIP(hipMemcpyAsync(d_req.p, requests, sizeof(eph_plot_request) * np_all, hipMemcpyHostToDevice, s));
        EPH_HIP(hipMemcpyAsync(d_lane_plot.p, lane_plot.data(), sizeof(long long) * np_all, hipMemcpyHostToDevice, s));
        EPH_HIP(hipMemcpyAsync(d_lane_col.p, lane_col.data(), sizeof(int) * np_all, hipMemcpyHostToDevice, s));
        CraftPlotArgs a{};
        a.n = b->n; a.max_knots = b->max_knots; a.nknots = b->nknots.p; a.perm = dealt ? b->perm.p : nullptr;
        a.knot_t = b->knot_t.p; a.knot_y = b->knot_y.p;
        a.table = {b->eph->bodies.p, b->eph->coeffs.p, b->eph->ncoef.p};
        a.req = d_req.p; a.view = *view; a.capacity = capacity;
        a.out_t = d_t.p; a.out_xyz = d_xyz.p; a.out_count = d_cnt.p; a.out_status = d_st.p; a.out_failed_at = d_fail.p;
        // the staging buffer: t[lane][cap] | failed_at[lane] | count[lane] | xyz[lane][cap][3] | status[lane]
        static_assert(sizeof(long long) == sizeof(int64_t), "count type");
        double *stage_t = static_cast<double *>(stage.dev());
        double *stage_fail = stage_t + per_pass * cap;
        long long *stage_cnt = reinterpret_cast<long long *>(stage_fail + per_pass);
        float *stage_xyz = reinterpret_cast<float *>(stage_cnt + per_pass);
        int *stage_st = reinterpret_cast<int *>(stage_xyz + 3 * per_pass * cap);
        const char *host = static_cast<const char *>(stage.host());
        const char *dev0 = static_cast<const char *>(stage.dev());
        const double *host_t = reinterpret_cast<const double *>(host + (reinterpret_cast<const char *>(stage_t) - dev0));
        const double *host_fail = reinterpret_cast<const double *>(host + (reinterpret_cast<const char *>(stage_fail) - dev0));
        const long long *host_cnt = reinterpret_cast<const long long *>(host + (reinterpret_cast<const char *>(stage_cnt) - dev0));
        const float *host_xyz = reinterpret_cast<const float *>(host + (reinterpret_cast<const char *>(stage_xyz) - dev0));
        const int *host_st = reinterpret_cast<const int *>(host + (reinterpret_cast<const char *>(stage_st) - dev0));
        double kernel_ms = 0.0, copy_ms = 0.0;
        for (size_t l0 = 0; l0 < np_all; l0 += per_pass) {
            const size_t nl = std::min(per_pass, np_all - l0);
            a.n_lanes = (long long)nl;
            a.lane_plot = d_lane_plot.p + l0;
            a.lane_col = d_lane_col.p + l0;
            if (trace) EPH_HIP(hipEventRecord(b->ev0, s));
            hipLaunchKernelGGL(k_craft_plot_points, dim3((unsigned)((nl + 63) / 64)), dim3(64), 0, s, a);
            if ((he = hipGetLastError()) != hipSuccess) { set_last_error("k_craft_plot_points", he); return EPH_ERR_HIP; }
            if (trace) EPH_HIP(hipEventRecord(b->ev1, s));
            hipLaunchKernelGGL(k_craft_plot_rows_out, dim3((unsigned)nl), dim3(64), 0, s, (long long)nl, (long long)capacity,
                               (const double *)d_t.p, (const float *)d_xyz.p, (const long long *)d_cnt.p, (const int *)d_st.p,
                               (const double *)d_fail.p, stage_t, stage_xyz, stage_cnt, stage_st, stage_fail);
            if ((he = hipGetLastError()) != hipSuccess) { set_last_error("k_craft_plot_rows_out", he); return EPH_ERR_HIP; }
            EPH_HIP(hipStreamSynchronize(s));
            const auto c0 = std::chrono::steady_clock::now();
            for (size_t l = 0; l < nl; ++l) {
                const size_t p = (size_t)lane_plot[l0 + l];
                const size_t cnt = (size_t)std::min<long long>(std::max<long long>(host_cnt[l], 0), (long long)cap);
                out_count[p] = (int64_t)cnt;
                out_status[p] = host_st[l];
                out_failed_at[p] = host_fail[l];
                if (cnt) {
                    std::memcpy(out_t + p * cap, host_t + l * cap, sizeof(double) * cnt);
                    std::memcpy(out_xyz + p * cap * 3, host_xyz + l * cap * 3, sizeof(float) * 3 * cnt);
                }
            }
            if (trace) {
                float ms = 0.0f;
                EPH_HIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
                kernel_ms += ms;
                copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
            }
        }
        idle.disarm();
        if (trace)
            fprintf(stderr, "craft_plot: plots %lld capacity %lld passes %lld kernel_ms %.4f host_copy_ms %.4f\n", (long long)n_plots,
                    (long long)capacity, (long long)((np_all + per_pass - 1) / per_pass), kernel_ms, copy_ms);
        return EPH_OK;
    } catch (const std::bad_alloc &) { return EPH_ERR_OUT_OF_MEMORY; } catch (...) { return EPH_ERR_HIP; }
}

}  // extern "C"
#pragma GCC visibility pop
