// evaluators.hip -- evaluators that never touch a spacecraft batch: the debug window's interpolation-error scan of the bodies' table,
// CubicHermiteSpline evaluation at many epochs, the adaptive plot sampling and the closest-separation search.
//
// Mirrors (paths relative to the reference repository root):
//   the interpolation-error scan                        ephemeris_explorer/src/ui/windows/debug.rs:182-238
// The spline evaluations, the sampler and the search themselves (trajectory.rs, plot.rs, analysis.rs) are trajectory_eval.h's, with
// their line numbers.
#include <algorithm>
#include <vector>

#include "ephemeris_table.h"

namespace eph {

// The debug window's interpolation-error scan (ephemeris_explorer/src/ui/windows/debug.rs:182-238): re-integrate
// the massive bodies and, after every step, compare each body's position with its UniformSpline at that epoch;
// keep the maximum of `position.distance(traj_position) * 1e3` (metres) per body. Thread per body; err[b] < 0 marks
// "no entry yet" (EntityHashMap::entry(..).or_insert).
__global__ void __launch_bounds__(256) k_interp_error(int n, int npad, const double *__restrict__ Y, double t,
                                                      const BodyEntry *__restrict__ bodies,
                                                      const double *__restrict__ coeffs, const int *__restrict__ ncoef,
                                                      double *err, int *failed) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    V3 tp;
    if (!body_position(BodyTable{bodies, coeffs, ncoef}, b, t, tp)) { *failed = 1; return; }   // traj.position(epoch).unwrap()
    const V3 d = sub(V3{Y[b], Y[npad + b], Y[2 * npad + b]}, tp);
    const double e = sqrt(dot(d, d)) * 1e3;
    const double cur = err[b];
    err[b] = cur < 0.0 ? e : fmax(cur, e);
}

// CubicHermiteSpline::state_vector at many epochs; outside the spline: zeros and inside = 0
__global__ void __launch_bounds__(256) k_hermite_eval(long long nk, const double *__restrict__ t,
                                                      const double *__restrict__ pos, const double *__restrict__ vel,
                                                      long long m, const double *__restrict__ at,
                                                      double *__restrict__ op, double *__restrict__ ov,
                                                      uint8_t *__restrict__ inside) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    V3 p = {0.0, 0.0, 0.0}, v = {0.0, 0.0, 0.0};
    const bool ok = hermite_state_vector(KnotArrays{nk, t, pos, vel}, at[q], p, v);
    op[q * 3] = p.x; op[q * 3 + 1] = p.y; op[q * 3 + 2] = p.z;
    if (ov) { ov[q * 3] = v.x; ov[q * 3 + 1] = v.y; ov[q * 3 + 2] = v.z; }
    inside[q] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------
// Adaptive plot sampling (plot_sample, trajectory_eval.h), one thread per plotted trajectory: a body of the table or a range of
// the caller's knot arrays, points to [plot][k].
// ------------------------------------------------------------------------------------------------------
struct PlotArgs {
    long long n_plots;
    int n_bodies;
    BodyTable table;
    const eph_plot_request *req;
    eph_plot_view view;
    const double *knot_t, *knot_pos, *knot_vel;
    long long capacity;
    double *out_t;
    float *out_xyz;
    long long *out_count;
    int *out_status;
    double *out_failed_at;
};
struct PlotSource {           // body >= 0: that body of the table; otherwise the knots
    const BodyTable &table;
    int body;
    KnotArrays knots;
    __device__ __forceinline__ void bounds(double &start, double &end, long long &segs) const {
        if (body >= 0) {
            const BodyEntry be = table.bodies[body];
            start = be.start; end = be.start + be.span; segs = be.npoly;
        } else {
            hermite_bounds(knots, start, end, segs);
        }
    }
    __device__ __forceinline__ bool state_vector(double t, V3 &p, V3 &v) const {
        return body >= 0 ? body_state_vector(table, body, t, p, v) : hermite_state_vector(knots, t, p, v);
    }
};
struct PlotRowSink {          // one plot's row of the results, [plot][k], and its three scalars
    double *t;
    float *xyz;
    long long *n;
    int *st;
    double *fail;
    __device__ __forceinline__ void push(long long k, double at, V3 q) const {
        t[k] = at; xyz[3 * k] = (float)q.x; xyz[3 * k + 1] = (float)q.y; xyz[3 * k + 2] = (float)q.z;
    }
    __device__ __forceinline__ void count(long long np) const { *n = np; }
    __device__ __forceinline__ void status(int s) const { *st = s; }
    __device__ __forceinline__ void failed_at(double at) const { *fail = at; }
};

__global__ void __launch_bounds__(64) k_plot_points(const PlotArgs a) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_plots) return;
    const eph_plot_request rq = a.req[p];
    const PlotSource src = {a.table, rq.source_body,
                            KnotArrays{rq.knot_count, a.knot_t + rq.knot_first, a.knot_pos + 3 * rq.knot_first, a.knot_vel + 3 * rq.knot_first}};
    PlotRowSink sink = {a.out_t + p * a.capacity, a.out_xyz + p * a.capacity * 3, a.out_count + p, a.out_status + p, a.out_failed_at + p};
    plot_sample(a.table, a.view, rq, src, sink);
}

// ------------------------------------------------------------------------------------------------------
// The closest-separation search of target plotting (closest_separation, trajectory_eval.h), one thread per request: source and
// target are bodies of the table or ranges of the caller's knot arrays.
// ------------------------------------------------------------------------------------------------------
struct SeparationArgs {
    long long n_requests;
    BodyTable table;
    const eph_separation_request *req;
    const double *knot_t, *knot_pos, *knot_vel;
    uint8_t *out_found;
    double *out_time, *out_distance;
    int *out_iterations, *out_status;
    double *out_failed_at;
};

__global__ void __launch_bounds__(64) k_closest_separation(const SeparationArgs a) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_requests) return;
    const eph_separation_request rq = a.req[p];
    auto knots = [&](long long first, long long count) {
        return KnotArrays{count, a.knot_t + first, a.knot_pos + 3 * first, a.knot_vel + 3 * first};
    };
    const SeparationTrajectory<KnotArrays> src = {a.table, rq.source_body, knots(rq.source_knot_first, rq.source_knot_count)};
    const SeparationTrajectory<KnotArrays> tgt = {a.table, rq.target_body, knots(rq.target_knot_first, rq.target_knot_count)};
    const Separation r = closest_separation(src, tgt, rq.left, rq.right, rq.precision, rq.max_iterations, rq.metric);
    a.out_found[p] = (uint8_t)r.found;
    a.out_time[p] = r.time;
    a.out_distance[p] = r.distance;
    a.out_iterations[p] = r.iterations;
    a.out_status[p] = r.status;
    a.out_failed_at[p] = r.failed_at;
}

}  // namespace eph

using namespace eph;

#pragma GCC visibility push(default)
extern "C" {

int32_t eph_ephemeris_interpolation_errors(const eph_ephemeris *e, eph_nbody *h, int64_t n_steps, double *max_error_m,
                                           int64_t *steps_done) {
    EPH_GUARD_BEGIN
        if (!e || !h || !h->p || n_steps < 0 || !max_error_m) return EPH_ERR_BAD_ARGUMENT;
        NBodyIntegration *g = h->p;
        const int n = g->n();
        if (n != e->n_bodies || g->sharded()) return EPH_ERR_BAD_ARGUMENT;
        std::shared_lock<std::shared_mutex> table_lock(e->mu);
        EPH_HIP(hipSetDevice(g->device()));
        DevBuf<double> err;
        DevBuf<int> failed;
        int st;
        if ((st = err.alloc(std::max(n, 1))) || (st = failed.alloc(1))) return st;
        std::vector<double> init((size_t)std::max(n, 1), -1.0);
        EPH_HIP(hipMemcpyAsync(err.p, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice, g->stream()));
        EPH_HIP(hipMemsetAsync(failed.p, 0, sizeof(int), g->stream()));
        EPH_HIP(hipStreamSynchronize(g->stream()));
        int64_t done = 0;
        int status = EPH_OK;
        const BodyTable table = body_table(e);
        for (; done < n_steps; ++done) {                       // while integrator.advance(&mut nbody).is_ok()
            if ((status = g->advance(1))) break;
            if (n > 0)
                hipLaunchKernelGGL(k_interp_error, dim3((n + 255) / 256), dim3(256), 0, g->stream(), n, g->npad(),
                                   g->positions_soa(), g->time(), table.bodies, table.coeffs, table.ncoef, err.p, failed.p);
        }
        hipError_t he = hipGetLastError();
        if (he != hipSuccess) { set_last_error("k_interp_error", he); return EPH_ERR_HIP; }
        int f = 0;
        EPH_HIP(hipMemcpyAsync(max_error_m, err.p, sizeof(double) * n, hipMemcpyDeviceToHost, g->stream()));
        EPH_HIP(hipMemcpyAsync(&f, failed.p, sizeof(int), hipMemcpyDeviceToHost, g->stream()));
        EPH_HIP(hipStreamSynchronize(g->stream()));
        if (steps_done) *steps_done = done;
        if (status < 0) return status;
        if (f) return EPH_EVAL_FAILED;                         // an epoch outside a spline: the reference would panic
        return EPH_OK;                                         // a StepError (bound reached) just ends the scan
    EPH_GUARD_END
}

int32_t eph_hermite_eval(int64_t nknots, const double *t, const double *pos, const double *vel, int64_t m,
                         const double *at, double *op, double *ov, uint8_t *inside) {
    EPH_GUARD_BEGIN
        if (nknots < 0 || m < 0 || (m > 0 && (!at || !op || !inside)) || (nknots > 0 && (!t || !pos || !vel)))
            return EPH_ERR_BAD_ARGUMENT;
        int st = check_device();
        if (st) return st;
        if (m == 0) return EPH_OK;
        const size_t nk = (size_t)nknots;
        DevBuf<double> dt, dp, dv, dat, dop, dov;
        DevBuf<uint8_t> din;
        if ((st = upload(dt, t, nk)) || (st = upload(dp, pos, 3 * nk)) || (st = upload(dv, vel, 3 * nk)) || (st = upload(dat, at, (size_t)m)) ||
            (st = dop.alloc(3 * (size_t)m)) || (st = dov.alloc(3 * (size_t)m)) || (st = din.alloc(m)))
            return st;
        EPH_LAUNCH("k_hermite_eval", k_hermite_eval, dim3((unsigned)((m + 255) / 256)), dim3(256), nullptr, (long long)nknots,
                   dt.p, dp.p, dv.p, (long long)m, dat.p, dop.p, ov ? dov.p : nullptr, din.p);
        EPH_HIP(hipMemcpy(op, dop.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost));
        if (ov) EPH_HIP(hipMemcpy(ov, dov.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(inside, din.p, m, hipMemcpyDeviceToHost));
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_plot_points(const eph_ephemeris *e, const eph_plot_view *view, int64_t n_plots, const eph_plot_request *requests,
                        int64_t n_knots, const double *knot_t, const double *knot_pos, const double *knot_vel,
                        int64_t capacity, double *out_t, float *out_xyz, int64_t *out_count, int32_t *out_status,
                        double *out_failed_at) {
    EPH_GUARD_BEGIN
        if (!e || !view || n_plots < 0 || n_knots < 0 || capacity < 0 || (n_plots > 0 && (!requests || !out_count || !out_status || !out_failed_at)) ||
            (n_knots > 0 && (!knot_t || !knot_pos || !knot_vel)) || (n_plots > 0 && capacity > 0 && (!out_t || !out_xyz)))
            return EPH_ERR_BAD_ARGUMENT;
        for (int64_t p = 0; p < n_plots; ++p) {
            const eph_plot_request &r = requests[p];
            if (r.source_body >= e->n_bodies || r.reference_body >= e->n_bodies || r.reference_body < -1 || r.source_body < -1 ||
                r.max_points < 0 || r.max_points > capacity || r.bound < 0 || r.bound > 2)
                return EPH_ERR_BAD_ARGUMENT;
            if (r.source_body < 0 && (r.knot_first < 0 || r.knot_count < 0 || r.knot_first + r.knot_count > n_knots))
                return EPH_ERR_BAD_ARGUMENT;
        }
        int st = check_device();
        if (st) return st;
        if (n_plots == 0) return EPH_OK;
        std::shared_lock<std::shared_mutex> table_lock(e->mu);
        EPH_HIP(hipSetDevice(e->device));
        const size_t nk = (size_t)n_knots, np = (size_t)n_plots, cap = (size_t)std::max<int64_t>(capacity, 1);
        DevBuf<eph_plot_request> d_req;
        DevBuf<double> d_kt, d_kp, d_kv, d_t, d_fail;
        DevBuf<float> d_xyz;
        DevBuf<long long> d_cnt;
        DevBuf<int> d_st;
        if ((st = upload(d_req, requests, np)) || (st = upload(d_kt, knot_t, nk)) || (st = upload(d_kp, knot_pos, 3 * nk)) ||
            (st = upload(d_kv, knot_vel, 3 * nk)) || (st = d_t.alloc(np * cap)) || (st = d_xyz.alloc(3 * np * cap)) ||
            (st = d_cnt.alloc(np)) || (st = d_st.alloc(np)) || (st = d_fail.alloc(np)))
            return st;
        PlotArgs a{};
        a.n_plots = n_plots; a.n_bodies = e->n_bodies;
        a.table = body_table(e);
        a.req = d_req.p; a.view = *view;
        a.knot_t = d_kt.p; a.knot_pos = d_kp.p; a.knot_vel = d_kv.p;
        a.capacity = capacity; a.out_t = d_t.p; a.out_xyz = d_xyz.p; a.out_count = d_cnt.p; a.out_status = d_st.p;
        a.out_failed_at = d_fail.p;
        EPH_LAUNCH("k_plot_points", k_plot_points, dim3((unsigned)((n_plots + 63) / 64)), dim3(64), nullptr, a);
        static_assert(sizeof(long long) == sizeof(int64_t), "count type");
        EPH_HIP(hipMemcpy(out_count, d_cnt.p, sizeof(int64_t) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_status, d_st.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_failed_at, d_fail.p, sizeof(double) * np, hipMemcpyDeviceToHost));
        if (capacity > 0) {
            EPH_HIP(hipMemcpy(out_t, d_t.p, sizeof(double) * np * cap, hipMemcpyDeviceToHost));
            EPH_HIP(hipMemcpy(out_xyz, d_xyz.p, sizeof(float) * 3 * np * cap, hipMemcpyDeviceToHost));
        }
        return EPH_OK;
    EPH_GUARD_END
}

int32_t eph_closest_separation(const eph_ephemeris *e, int64_t n_requests, const eph_separation_request *requests,
                               int64_t n_knots, const double *knot_t, const double *knot_pos, const double *knot_vel,
                               uint8_t *out_found, double *out_time, double *out_distance, int32_t *out_iterations,
                               int32_t *out_status, double *out_failed_at) {
    EPH_GUARD_BEGIN
        if (!e || n_requests < 0 || n_knots < 0 ||
            (n_requests > 0 && (!requests || !out_found || !out_time || !out_distance || !out_iterations || !out_status || !out_failed_at)) ||
            (n_knots > 0 && (!knot_t || !knot_pos || !knot_vel)))
            return EPH_ERR_BAD_ARGUMENT;
        auto slice_ok = [&](int32_t body, int64_t first, int64_t count) {
            return body >= 0 || (first >= 0 && count >= 0 && first <= n_knots && count <= n_knots - first);
        };
        for (int64_t p = 0; p < n_requests; ++p) {
            const eph_separation_request &r = requests[p];
            if (r.source_body < -1 || r.source_body >= e->n_bodies || r.target_body < -1 || r.target_body >= e->n_bodies ||
                !slice_ok(r.source_body, r.source_knot_first, r.source_knot_count) ||
                !slice_ok(r.target_body, r.target_knot_first, r.target_knot_count) || !separation_request_ok(r))
                return EPH_ERR_BAD_ARGUMENT;
        }
        int st = check_device();
        if (st) return st;
        if (n_requests == 0) return EPH_OK;
        std::shared_lock<std::shared_mutex> table_lock(e->mu);
        EPH_HIP(hipSetDevice(e->device));
        const size_t nk = (size_t)n_knots, np = (size_t)n_requests;
        DevBuf<eph_separation_request> d_req;
        DevBuf<double> d_kt, d_kp, d_kv, d_time, d_dist, d_fail;
        DevBuf<uint8_t> d_found;
        DevBuf<int> d_it, d_st;
        if ((st = upload(d_req, requests, np)) || (st = upload(d_kt, knot_t, nk)) || (st = upload(d_kp, knot_pos, 3 * nk)) ||
            (st = upload(d_kv, knot_vel, 3 * nk)) || (st = d_found.alloc(np)) || (st = d_time.alloc(np)) || (st = d_dist.alloc(np)) || (st = d_it.alloc(np)) ||
            (st = d_st.alloc(np)) || (st = d_fail.alloc(np)))
            return st;
        SeparationArgs a{};
        a.n_requests = n_requests;
        a.table = body_table(e);
        a.req = d_req.p;
        a.knot_t = d_kt.p; a.knot_pos = d_kp.p; a.knot_vel = d_kv.p;
        a.out_found = d_found.p; a.out_time = d_time.p; a.out_distance = d_dist.p; a.out_iterations = d_it.p; a.out_status = d_st.p;
        a.out_failed_at = d_fail.p;
        EPH_LAUNCH("k_closest_separation", k_closest_separation, dim3((unsigned)((n_requests + 63) / 64)), dim3(64), nullptr, a);
        EPH_HIP(hipMemcpy(out_found, d_found.p, np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_time, d_time.p, sizeof(double) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_distance, d_dist.p, sizeof(double) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_iterations, d_it.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_status, d_st.p, sizeof(int32_t) * np, hipMemcpyDeviceToHost));
        EPH_HIP(hipMemcpy(out_failed_at, d_fail.p, sizeof(double) * np, hipMemcpyDeviceToHost));
        return EPH_OK;
    EPH_GUARD_END
}

}  // extern "C"
#pragma GCC visibility pop
