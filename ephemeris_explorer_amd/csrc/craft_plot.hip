// craft_plot.hip -- the adaptive plot sampler on the knot slabs of a spacecraft batch (eph_craft_batch_plot_points): what
// eph_plot_points computes for a ship's knots, with the knots read where the sweep left them. Reads the batch; changes nothing in it.
//
// Mirrors (paths relative to the reference repository root):
//   compute_plot_points_parallel, PlotPoints::new, angular_distance   ephemeris_explorer/src/ui/world/plot.rs:93-149,272-374,429-436
//   CubicHermiteSpline::state_vector, RelativeTrajectory, UniformSpline::state_vector   ephemeris/src/trajectory.rs:277-334,449-470,766-797
// The arithmetic of one evaluation restates k_plot_points' device functions (evaluators.hip) operation for operation -- that unit is
// left as it is -- with the knot source replaced by one column of the slabs (craft_eval.hip's addressing).
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
    const BodyEntry *bodies;
    const double *coeffs;
    const int *ncoef;
    const eph_plot_request *req;    // [plot]
    eph_plot_view view;
    long long capacity;
    double *out_t;                  // [k][lane]
    float *out_xyz;                 // [k][3][lane]
    long long *out_count;           // [lane]
    int *out_status;
    double *out_failed_at;
};

// UniformSpline::state_vector / position of body b  (trajectory.rs:449-470): plot_body_sv / plot_body_pos of evaluators.hip
__device__ bool craft_plot_body_sv(const CraftPlotArgs &a, int b, double t, V3 &pos, V3 &vel) {
    const BodyEntry be = a.bodies[b];
    long long idx;
    double tau;
    if (!spline_locate(be, t, idx, tau)) return false;
    const double *co = a.coeffs + (be.coeff_off + idx) * kDiv * 3;
    const int nc = a.ncoef[be.coeff_off + idx];
    double rp[3], rv[3];
    for (int c = 0; c < 3; ++c) {                     // Polynomial::eval_and_deriv
        const double first = nc ? co[c] : 0.0;
        const double last = nc ? co[(nc - 1) * 3 + c] : 0.0;
        double e = last, d = last;
        for (int k = nc - 2; k >= 1; --k) {
            e = e * tau + co[k * 3 + c];
            d = d * tau + e;
        }
        e = e * tau + first;
        rp[c] = e;
        rv[c] = d / be.interval;
    }
    pos = {rp[0], rp[1], rp[2]};
    vel = {rv[0], rv[1], rv[2]};
    return true;
}
__device__ bool craft_plot_body_pos(const CraftPlotArgs &a, int b, double t, V3 &out) {
    const BodyEntry be = a.bodies[b];
    long long idx;
    double tau;
    if (!spline_locate(be, t, idx, tau)) return false;
    const double *co = a.coeffs + (be.coeff_off + idx) * kDiv * 3;
    const int nc = a.ncoef[be.coeff_off + idx];
    V3 bp = {0.0, 0.0, 0.0};
    for (int k = nc - 1; k >= 0; --k) {               // Polynomial::eval (Horner)
        bp.x = bp.x * tau + co[k * 3 + 0];
        bp.y = bp.y * tau + co[k * 3 + 1];
        bp.z = bp.z * tau + co[k * 3 + 2];
    }
    out = bp;
    return true;
}

// CubicHermiteSpline::state_vector (trajectory.rs:766-797) on knots [0, nk) of one slab column: kt / ky point at the column, n is
// the stride of a knot row. One search path, the reference's binary search over the whole column per evaluation. A search that
// starts at the segment of the plot's last accepted point (gallop forward, then bisect; the same answer, because a column's knot
// epochs are strictly increasing -- every knot is the end t + h of an accepted step with h > 0, a restart keeps a prefix and appends
// later steps, a drain keeps the newest knot only -- so binary_search_by has one possible answer, and the sampler never evaluates
// below its last accepted epoch) was measured at 13 000 knots per ship and lost by 1-10 %: the upper levels of the search stay in
// cache, and the loop's time is the chain of fp64 divisions and square roots of one trial, not its loads
// (profiles/craft_plot.md, scripts/experiments/craft_plot_variants.patch).
__device__ __forceinline__ bool craft_plot_hermite_sv(long long nk, long long n, const double *__restrict__ kt,
                                                      const double *__restrict__ ky, double x, V3 &p, V3 &v) {
    long long lo = 0, hi = nk, hit = -1;
    while (lo < hi) {                                 // binary_search_by(|(t, _)| t.cmp(&at))
        const long long mid = lo + (hi - lo) / 2;
        const double tm = kt[mid * n];
        if (tm == x) { hit = mid; break; }
        if (tm < x) lo = mid + 1; else hi = mid;
    }
    if (hit >= 0) {
        p = {ky[(hit * 6 + 0) * n], ky[(hit * 6 + 1) * n], ky[(hit * 6 + 2) * n]};
        v = {ky[(hit * 6 + 3) * n], ky[(hit * 6 + 4) * n], ky[(hit * 6 + 5) * n]};
        return true;
    }
    if (lo == 0 || lo >= nk) return false;            // i.checked_sub(1)? / self.0.get(i + 1)?
    const long long i = lo - 1;
    const double b0 = kt[i * n], dt = kt[(i + 1) * n] - b0;
    const double dt_recip = 1.0 / dt;
    const double dt_recip_2 = dt_recip * dt_recip;
    const double dt_recip_3 = dt_recip * dt_recip_2;
    const double s = x - b0;
    double op[3], ov[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v0 = ky[(i * 6 + c) * n], v1 = ky[((i + 1) * 6 + c) * n];
        const double d0 = ky[(i * 6 + 3 + c) * n], d1 = ky[((i + 1) * 6 + 3 + c) * n];
        const double dt_val = v1 - v0;
        const double a2 = dt_val * dt_recip_2 * 3.0 - (d0 * 2.0 + d1) * dt_recip;
        const double a3 = dt_val * dt_recip_3 * -2.0 + (d0 + d1) * dt_recip_2;
        op[c] = (((a3 * s + a2) * s) + d0) * s + v0;
        ov[c] = ((a3 * s * 3.0 + a2 * 2.0) * s) + d0;
    }
    p = {op[0], op[1], op[2]};
    v = {ov[0], ov[1], ov[2]};
    return true;
}
// glam DMat3::mul_vec3: ((x_axis * v.x) + (y_axis * v.y)) + (z_axis * v.z)   (glam 0.30.10)
__device__ __forceinline__ V3 craft_plot_mat3_mul(const double (&m)[9], V3 v) {
    const V3 x = {m[0], m[1], m[2]}, y = {m[3], m[4], m[5]}, z = {m[6], m[7], m[8]};
    return add(add(scale(x, v.x), scale(y, v.y)), scale(z, v.z));
}
// angular_distance  plot.rs:429-436: DVec3::normalize = self * self.length().recip()
__device__ __forceinline__ double craft_plot_angular_distance(V3 cam, V3 p1, V3 p2) {
    const V3 d1 = sub(p1, cam), d2 = sub(p2, cam);
    const V3 v1 = scale(d1, length_recip(d1)), v2 = scale(d2, length_recip(d2));
    const V3 w = cross(v1, v2);
    const double d = dot(v1, v2);
    return dot(w, w) / (d * d);
}
__device__ __forceinline__ double craft_plot_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// One lane per plot, k_plot_points' sequential adaptive loop. The lanes of a pass are ordered by slab column (the host sorts them):
// craft that were dealt to neighbouring columns have similar time scales, so a wave's lanes ask for similar knot indices at similar
// epochs -- few cache lines per load -- and take similar numbers of points. 124 VGPRs (128 allocated), no scratch, 4 waves per SIMD.
__global__ void __launch_bounds__(64) k_craft_plot_points(const CraftPlotArgs a) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= a.n_lanes) return;
    const eph_plot_request rq = a.req[a.lane_plot[lane]];
    a.out_count[lane] = 0;
    a.out_status[lane] = EPH_OK;
    a.out_failed_at[lane] = 0.0;
    const long long n = a.n, col = a.lane_col[lane];
    const long long craft = a.perm ? a.perm[col] : col;
    const long long nk = min(max(a.nknots[craft], 0), a.max_knots);
    const double *__restrict__ kt = a.knot_t + col;
    const double *__restrict__ ky = a.knot_y + col;
    // RelativeTrajectory bounds / segment count  trajectory.rs:277-308
    double start = nk > 0 ? kt[0] : -1.7976931348623157e308;        // Epoch::MIN / MAX of an empty spline :756-763
    double end = nk > 0 ? kt[(nk - 1) * n] : 1.7976931348623157e308;
    long long segs = nk > 0 ? nk - 1 : 0;
    double rstart = 0.0, rend = 0.0;
    if (rq.reference_body >= 0) {
        const BodyEntry rb = a.bodies[rq.reference_body];
        rstart = rb.start; rend = rb.start + rb.span;
        start = rstart < start ? start : rstart;                    // Ord::max / Ord::min
        end = rend < end ? rend : end;
        segs = rb.npoly < segs ? rb.npoly : segs;
    }
    if (!rq.enabled || segs == 0 || start > end) return;            // plot.enabled && !relative.is_empty()  :324
    const double current = a.view.current;
    const double current_clamped = craft_plot_clamp(current, start, end);
    double tmin = craft_plot_clamp(rq.start, start, end), tmax = craft_plot_clamp(rq.end, start, end);
    if (rq.bound == 1) tmin = current_clamped < tmin ? tmin : current_clamped;      // min.max(current_clamped)
    else if (rq.bound == 2) tmax = current_clamped < tmax ? current_clamped : tmax; // max.min(current_clamped)
    if (tmin >= tmax) return;
    // translation: reference.position(current.clamp(r.start(), r.end())).unwrap()  :355-361
    V3 tr = {0.0, 0.0, 0.0};
    if (rq.reference_body >= 0) {
        const double tc = craft_plot_clamp(current, rstart, rend);
        if (!craft_plot_body_pos(a, rq.reference_body, tc, tr)) { a.out_status[lane] = EPH_EVAL_FAILED; a.out_failed_at[lane] = tc; return; }
    }
    const V3 cam = {a.view.camera_position[0], a.view.camera_position[1], a.view.camera_position[2]};
    const V3 cell = {a.view.cell_offset[0], a.view.cell_offset[1], a.view.cell_offset[2]};
    const V3 gt = {a.view.grid_translation[0], a.view.grid_translation[1], a.view.grid_translation[2]};
    // |t| Some(root.to_global_sv(relative.state_vector(t)? + translation))
    auto eval = [&](double t, V3 &gp, V3 &gv) -> bool {
        V3 rp = {0.0, 0.0, 0.0}, rv = {0.0, 0.0, 0.0};              // reference first (trajectory.rs:329-333)
        if (rq.reference_body >= 0 && !craft_plot_body_sv(a, rq.reference_body, t, rp, rv)) return false;
        V3 sp, sv;
        if (!craft_plot_hermite_sv(nk, n, kt, ky, t, sp, sv)) return false;
        const V3 pos = add(sub(sp, rp), tr);
        const V3 vel = add(sub(sv, rv), V3{0.0, 0.0, 0.0});         // + StateVector::from_position(..).velocity
        gp = add(craft_plot_mat3_mul(a.view.grid_matrix3, sub(pos, cell)), gt);   // transform_point3(point - cell_to_float)
        gv = craft_plot_mat3_mul(a.view.grid_matrix3, vel);         // transform_vector3
        return true;
    };
    if (rq.max_points == 0) return;                                 // :101-103
    const double target = rq.tan2_angular_resolution * rq.tan2_angular_resolution;
    double previous_time = tmin;
    V3 ppos, pvel;
    if (!eval(previous_time, ppos, pvel)) { a.out_status[lane] = EPH_EVAL_FAILED; a.out_failed_at[lane] = previous_time; return; }
    double delta = tmax - previous_time;
    bool have_est = false;
    double estimated = 0.0;
    const long long nl = a.n_lanes;
    double *ot = a.out_t + lane;
    float *ox = a.out_xyz + lane;
    long long np = 0;
    auto push = [&](double t, V3 q) {
        ot[np * nl] = t;
        ox[(3 * np) * nl] = (float)q.x; ox[(3 * np + 1) * nl] = (float)q.y; ox[(3 * np + 2) * nl] = (float)q.z;
        ++np;
    };
    push(previous_time, ppos);
    while (previous_time < tmax && np < rq.max_points) {
        double t, next_error;
        V3 cpos, cvel;
        for (unsigned trial = 0;; ++trial) {
            if (have_est && estimated > 0.0) delta = delta * 0.9 * sqrt(sqrt(target / estimated));
            t = previous_time + delta;
            if (t > tmax) t = tmax;
            delta = t - previous_time;
            const V3 extrapolated = add(ppos, scale(pvel, delta));
            if (!eval(t, cpos, cvel)) { a.out_count[lane] = np; a.out_status[lane] = EPH_EVAL_FAILED; a.out_failed_at[lane] = t; return; }
            const double error = craft_plot_angular_distance(cam, extrapolated, cpos) / 16.0;
            if (error <= target) { next_error = error; break; }
            have_est = true;
            estimated = error;
            if (trial >= (1u << 20)) { a.out_count[lane] = np; a.out_status[lane] = EPH_MAX_ITERATIONS_REACHED; a.out_failed_at[lane] = t; return; }
        }
        previous_time = t;
        ppos = cpos;
        pvel = cvel;
        have_est = true;
        estimated = next_error;
        push(t, ppos);
    }
    a.out_count[lane] = np;
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
        const size_t n = (size_t)b->n, np_all = (size_t)n_plots, cap = (size_t)capacity;
        // lanes in slab-column order (a counting sort by column, stable in plot order); an undealt batch plotted craft by craft is in
        // that order already
        const bool dealt = !b->h_slot.empty();
        std::vector<long long> lane_plot(np_all);
        std::vector<int> lane_col(np_all);
        if (!dealt && !craft) {
            for (size_t p = 0; p < np_all; ++p) { lane_plot[p] = (long long)p; lane_col[p] = (int)p; }
        } else {
            auto column = [&](size_t p) { const size_t c = craft ? (size_t)craft[p] : p; return dealt ? (size_t)b->h_slot[c] : c; };
            std::vector<size_t> first(n + 1, 0);
            for (size_t p = 0; p < np_all; ++p) first[column(p) + 1] += 1;
            for (size_t c = 0; c < n; ++c) first[c + 1] += first[c];
            for (size_t p = 0; p < np_all; ++p) {
                const size_t c = column(p), l = first[c]++;
                lane_plot[l] = (long long)p; lane_col[l] = (int)c;
            }
        }
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
        a.bodies = b->eph->bodies.p; a.coeffs = b->eph->coeffs.p; a.ncoef = b->eph->ncoef.p;
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
