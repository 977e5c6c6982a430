// trajectory_eval.h -- the reference's trajectory evaluation, its adaptive plot sampling and its closest-separation search, each
// operation stated once for every device unit: a UniformSpline given by its table entry, a body of the live table, a
// CubicHermiteSpline over knots wherever they lie, the plot sampler and the search over any such trajectory. Every function restates
// the reference's operation order bit for bit (-ffp-contract=off; the association of every expression is the reference's): a
// correction is made here and nowhere else.
// Device code only (but separation_request_ok, the host's check of what both searches refuse), every function inlined into its
// kernel. Not here, on purpose: the sweep's own body loop, whose parts are stated once each where they are used (craft_device.h:
// spline_locate_fast, the guarded lookup; craft_sweep.hip: locate_spec, the speculative one, and horner_all / horner_row over all
// kDiv rows), k_craft_tau (approximate by design) and the event search's struct Hermite (craft_events.hip: coefficients built once
// per step, evaluated many times).
//
// Mirrors (paths relative to the reference repository root):
//   UniformSpline::{position, state_vector, get_polynomial}, Polynomial::{eval, eval_and_deriv}, eval_slice_horner
//                                                                     ephemeris/src/trajectory.rs:368-385,398-410,449-470,551-617
//   CubicHermite::{new, eval, eval_derivative}, CubicHermiteSpline::{start, end, state_vector}
//                                                                     ephemeris/src/trajectory.rs:645-696,756-797
//   RelativeTrajectory::{start, end, len, state_vector}              ephemeris/src/trajectory.rs:277-334
//   compute_plot_points_parallel, PlotPoints::new, angular_distance   ephemeris_explorer/src/ui/world/plot.rs:93-149,272-374,429-436
//   RelativeTrajectory::closest_separation_between                   ephemeris/src/trajectory.rs:202-248
//   Trajectory::{distance_squared_at, distance_at}                   ephemeris_explorer/src/dynamics/mod.rs:133-146
//   setup_target_plotting (the search's caller and PlotSeparation)   ephemeris_explorer/src/analysis.rs:344-366
// glam::DVec3 / DMat3 operations (crate glam 0.30.10, not on disk) are restated from the published crate.
#pragma once
#include "craft_device.h"

namespace eph {

// ---- a UniformSpline: its table entry, and the coefficient rows [poly][kDiv][3] and counts [poly] that the entry's coeff_off indexes ---
// (the polynomial's loops stay inside these two functions: with Polynomial::eval_and_deriv as a function of its own under
// spline_state_vector, both forms of k_craft_events allocate two VGPRs more, 130 where 128 is the last count that fits four waves)
// UniformSpline::position :449-457 with Polynomial::eval (eval_slice_horner :398-410); false = None
__device__ __forceinline__ bool spline_position(const BodyEntry &be, const double *coeffs, const int *ncoef, double t, V3 &out) {
    long long idx;
    double tau;
    if (!spline_locate(be, t, idx, tau)) return false;
    const double *co = coeffs + (be.coeff_off + idx) * kDiv * 3;
    const int nc = ncoef[be.coeff_off + idx];
    V3 bp = {0.0, 0.0, 0.0};
    for (int k = nc - 1; k >= 0; --k) {               // Polynomial::eval (Horner)
        bp.x = bp.x * tau + co[k * 3 + 0];
        bp.y = bp.y * tau + co[k * 3 + 1];
        bp.z = bp.z * tau + co[k * 3 + 2];
    }
    out = bp;
    return true;
}
// UniformSpline::state_vector :459-470 with Polynomial::eval_and_deriv :368-385 (velocity = derivative / interval); false = None
__device__ __forceinline__ bool spline_state_vector(const BodyEntry &be, const double *coeffs, const int *ncoef, double t, V3 &pos, V3 &vel) {
    long long idx;
    double tau;
    if (!spline_locate(be, t, idx, tau)) return false;
    const double *co = coeffs + (be.coeff_off + idx) * kDiv * 3;
    const int nc = ncoef[be.coeff_off + idx];
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

// ---- a body of the live table --------------------------------------------------------------------------------------------------
struct BodyTable {            // what an evaluation reads of eph_ephemeris (under its lock)
    const BodyEntry *bodies;
    const double *coeffs;
    const int *ncoef;
};
// body b's UniformSpline::position / ::state_vector; false = None
__device__ __forceinline__ bool body_position(const BodyTable &tb, int b, double t, V3 &out) {
    const BodyEntry be = tb.bodies[b];
    return spline_position(be, tb.coeffs, tb.ncoef, t, out);
}
__device__ __forceinline__ bool body_state_vector(const BodyTable &tb, int b, double t, V3 &pos, V3 &vel) {
    const BodyEntry be = tb.bodies[b];
    return spline_state_vector(be, tb.coeffs, tb.ncoef, t, pos, vel);
}

// ---- a CubicHermiteSpline over knots [0, nk): Knots gives nk, t(k) and component d of knot k, y(k, d) (0-2 position, 3-5 velocity) ---
struct KnotArrays {           // the caller's arrays: t[k], pos[k][3], vel[k][3]
    long long nk;
    const double *at, *pos, *vel;
    __device__ __forceinline__ double t(long long k) const { return at[k]; }
    __device__ __forceinline__ double y(long long k, int d) const { return d < 3 ? pos[k * 3 + d] : vel[k * 3 + d - 3]; }
};
struct KnotColumn {           // one column of a batch's knot slabs: kt / ky point at the column, n is the stride of a knot row
    long long nk, n;
    const double *__restrict__ kt;      // [k][column]
    const double *__restrict__ ky;      // [k][6][column]
    __device__ __forceinline__ double t(long long k) const { return kt[k * n]; }
    __device__ __forceinline__ double y(long long k, int d) const { return ky[(k * 6 + d) * n]; }
};
// CubicHermiteSpline::{start, end} :756-763 and its segment count
template <class Knots>
__device__ __forceinline__ void hermite_bounds(const Knots &kn, double &start, double &end, long long &segs) {
    start = kn.nk > 0 ? kn.t(0) : -1.7976931348623157e308;          // Epoch::MIN / MAX of an empty spline
    end = kn.nk > 0 ? kn.t(kn.nk - 1) : 1.7976931348623157e308;
    segs = kn.nk > 0 ? kn.nk - 1 : 0;
}
// CubicHermiteSpline::state_vector :766-797 with CubicHermite::{new, eval, eval_derivative} :645-696; false = None.
// One search path, the reference's binary search over all the knots per evaluation. A search that starts at the segment of the
// caller's last evaluation (gallop forward, then bisect; the same answer on a slab column, because a column's knot epochs are
// strictly increasing -- every knot is the end t + h of an accepted step with h > 0, a restart keeps a prefix and appends later
// steps, a drain keeps the newest knot only -- so binary_search_by has one possible answer) was measured twice and dropped twice:
// under the plot sampler at 13 000 knots per ship it lost by 1-10 %, because the upper levels of the search stay in cache and the
// loop's time is the chain of fp64 divisions and square roots of one trial, not its loads (profiles/craft_plot.md,
// scripts/experiments/craft_plot_variants.patch); over ascending shared epochs in k_craft_eval it took 10 % off a kernel that is
// under 1 % of its call (profiles/craft_eval.md, scripts/experiments/craft_eval_gallop.patch).
template <class Knots>
__device__ __forceinline__ bool hermite_state_vector(const Knots &kn, double x, V3 &p, V3 &v) {
    long long lo = 0, hi = kn.nk, hit = -1;
    while (lo < hi) {                                 // binary_search_by(|(t, _)| t.cmp(&at))
        const long long mid = lo + (hi - lo) / 2;
        const double tm = kn.t(mid);
        if (tm == x) { hit = mid; break; }
        if (tm < x) lo = mid + 1; else hi = mid;
    }
    if (hit >= 0) {
        p = {kn.y(hit, 0), kn.y(hit, 1), kn.y(hit, 2)};
        v = {kn.y(hit, 3), kn.y(hit, 4), kn.y(hit, 5)};
        return true;
    }
    if (lo == 0 || lo >= kn.nk) return false;         // i.checked_sub(1)? / self.0.get(i + 1)?
    const long long i = lo - 1;
    const double b0 = kn.t(i), dt = kn.t(i + 1) - b0;
    const double dt_recip = 1.0 / dt;
    const double dt_recip_2 = dt_recip * dt_recip;
    const double dt_recip_3 = dt_recip * dt_recip_2;
    const double s = x - b0;
    double op[3], ov[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v0 = kn.y(i, c), v1 = kn.y(i + 1, c);
        const double d0 = kn.y(i, 3 + c), d1 = kn.y(i + 1, 3 + c);
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

// ---- the adaptive plot sampler -------------------------------------------------------------------------------------------------
// glam DMat3::mul_vec3: ((x_axis * v.x) + (y_axis * v.y)) + (z_axis * v.z)   (glam 0.30.10)
__device__ __forceinline__ V3 mat3_mul(const double (&m)[9], V3 v) {
    const V3 x = {m[0], m[1], m[2]}, y = {m[3], m[4], m[5]}, z = {m[6], m[7], m[8]};
    return add(add(scale(x, v.x), scale(y, v.y)), scale(z, v.z));
}
// angular_distance  plot.rs:429-436: DVec3::normalize = self * self.length().recip()
__device__ __forceinline__ double angular_distance(V3 cam, V3 p1, V3 p2) {
    const V3 d1 = sub(p1, cam), d2 = sub(p2, cam);
    const V3 v1 = scale(d1, length_recip(d1)), v2 = scale(d2, length_recip(d2));
    const V3 w = cross(v1, v2);
    const double d = dot(v1, v2);
    return dot(w, w) / (d * d);
}
__device__ __forceinline__ double ord_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// PlotPoints::new + compute_plot_points_parallel (plot.rs:93-149,272-374) of one plotted trajectory, sequentially: the source
// relative to the request's reference body, inside the request's window, in the view's grid frame.
//   Source: bounds(start, end, segments) of the trajectory and state_vector(t, p, v) (false = None).
//   Sink:   push(k, t, point) for point k, and the three result scalars count(n), status(s), failed_at(t).
// Points at or beyond the final count are never pushed.
template <class Source, class Sink>
__device__ __forceinline__ void plot_sample(const BodyTable &tb, const eph_plot_view &view, const eph_plot_request &rq,
                                            const Source &src, Sink &out) {
    out.count(0);
    out.status(EPH_OK);
    out.failed_at(0.0);
    // RelativeTrajectory bounds / segment count  trajectory.rs:277-308
    double start, end;
    long long segs;
    src.bounds(start, end, segs);
    double rstart = 0.0, rend = 0.0;
    if (rq.reference_body >= 0) {
        const BodyEntry rb = tb.bodies[rq.reference_body];
        rstart = rb.start; rend = rb.start + rb.span;
        start = rstart < start ? start : rstart;                    // Ord::max / Ord::min
        end = rend < end ? rend : end;
        segs = rb.npoly < segs ? rb.npoly : segs;
    }
    if (!rq.enabled || segs == 0 || start > end) return;            // plot.enabled && !relative.is_empty()  :324
    const double current = view.current;
    const double current_clamped = ord_clamp(current, start, end);
    double tmin = ord_clamp(rq.start, start, end), tmax = ord_clamp(rq.end, start, end);
    if (rq.bound == 1) tmin = current_clamped < tmin ? tmin : current_clamped;      // min.max(current_clamped)
    else if (rq.bound == 2) tmax = current_clamped < tmax ? current_clamped : tmax; // max.min(current_clamped)
    if (tmin >= tmax) return;
    // translation: reference.position(current.clamp(r.start(), r.end())).unwrap()  :355-361
    V3 tr = {0.0, 0.0, 0.0};
    if (rq.reference_body >= 0) {
        const double tc = ord_clamp(current, rstart, rend);
        if (!body_position(tb, rq.reference_body, tc, tr)) { out.status(EPH_EVAL_FAILED); out.failed_at(tc); return; }
    }
    const V3 cam = {view.camera_position[0], view.camera_position[1], view.camera_position[2]};
    const V3 cell = {view.cell_offset[0], view.cell_offset[1], view.cell_offset[2]};
    const V3 gt = {view.grid_translation[0], view.grid_translation[1], view.grid_translation[2]};
    // |t| Some(root.to_global_sv(relative.state_vector(t)? + translation))
    auto eval = [&](double t, V3 &gp, V3 &gv) -> bool {
        V3 rp = {0.0, 0.0, 0.0}, rv = {0.0, 0.0, 0.0};              // reference first (trajectory.rs:329-333)
        if (rq.reference_body >= 0 && !body_state_vector(tb, rq.reference_body, t, rp, rv)) return false;
        V3 sp, sv;
        if (!src.state_vector(t, sp, sv)) return false;
        const V3 pos = add(sub(sp, rp), tr);
        const V3 vel = add(sub(sv, rv), V3{0.0, 0.0, 0.0});         // + StateVector::from_position(..).velocity
        gp = add(mat3_mul(view.grid_matrix3, sub(pos, cell)), gt);  // transform_point3(point - cell_to_float)
        gv = mat3_mul(view.grid_matrix3, vel);                      // transform_vector3
        return true;
    };
    if (rq.max_points == 0) return;                                 // :101-103
    const double target = rq.tan2_angular_resolution * rq.tan2_angular_resolution;
    double previous_time = tmin;
    V3 ppos, pvel;
    if (!eval(previous_time, ppos, pvel)) { out.status(EPH_EVAL_FAILED); out.failed_at(previous_time); return; }
    double delta = tmax - previous_time;
    bool have_est = false;
    double estimated = 0.0;
    long long np = 0;
    out.push(np++, previous_time, ppos);
    while (previous_time < tmax && np < rq.max_points) {
        double t, next_error;
        V3 cpos, cvel;
        for (unsigned trial = 0;; ++trial) {
            if (have_est && estimated > 0.0) delta = delta * 0.9 * sqrt(sqrt(target / estimated));
            t = previous_time + delta;
            if (t > tmax) t = tmax;
            delta = t - previous_time;
            const V3 extrapolated = add(ppos, scale(pvel, delta));
            if (!eval(t, cpos, cvel)) { out.count(np); out.status(EPH_EVAL_FAILED); out.failed_at(t); return; }
            const double error = angular_distance(cam, extrapolated, cpos) / 16.0;
            if (error <= target) { next_error = error; break; }
            have_est = true;
            estimated = error;
            if (trial >= (1u << 20)) { out.count(np); out.status(EPH_MAX_ITERATIONS_REACHED); out.failed_at(t); return; }
        }
        previous_time = t;
        ppos = cpos;
        pvel = cvel;
        have_est = true;
        estimated = next_error;
        out.push(np++, t, ppos);
    }
    out.count(np);
}

// ---- the closest-separation search (target plotting) ----------------------------------------------------------------------------
struct Separation {           // what one search returns
    int found;                      // 1 = Some(time), 0 = None or a failure
    double time;                    // the epoch of closest separation
    double distance;                // PlotSeparation.distance at that epoch
    int iterations;                 // the value of the loop counter i at return
    int status;                     // EPH_OK; EPH_EVAL_FAILED: the reference unwraps a None position at failed_at
    double failed_at;
};
// What a search cannot run with, for both entry points: a metric outside 0..1, a NaN window, an iteration cap outside 0 .. 2^20.
inline bool separation_request_ok(const eph_separation_request &r) {
    return (r.metric == 0 || r.metric == 1) && r.left == r.left && r.right == r.right && r.max_iterations >= 0 &&
           r.max_iterations <= (1LL << 20);
}
// A trajectory of the search: body >= 0: that body of the table (bounds as plot_sample takes them from the BodyEntry); otherwise the
// CubicHermiteSpline over `knots`, whose ::position is the position half of ::state_vector (the same operations, a knot hit included).
template <class Knots>
struct SeparationTrajectory {
    const BodyTable &table;
    int body;
    Knots knots;
    __device__ __forceinline__ void bounds(double &start, double &end) const {
        if (body >= 0) {
            const BodyEntry be = table.bodies[body];
            start = be.start; end = be.start + be.span;
        } else {
            long long segs;
            hermite_bounds(knots, start, end, segs);
        }
    }
    __device__ __forceinline__ bool position(double t, V3 &p) const {
        if (body >= 0) return body_position(table, body, t, p);
        V3 v;
        return hermite_state_vector(knots, t, p, v);
    }
};
// RelativeTrajectory::closest_separation_between (trajectory.rs:202-248) of `src` relative to `tgt` with one of the app's two
// distance closures, then PlotSeparation.distance (analysis.rs:362-366).
//   Source, Target: bounds(start, end) of the trajectory and position(t, p) (false = None).
//   metric 0: Trajectory::distance_squared_at, 1: Trajectory::distance_at (dynamics/mod.rs:133-146): source position first, then
//   the target's; glam distance_squared = (a - b).length_squared() = (x*x + y*y) + z*z, distance = its sqrt.
// Epoch / Duration arithmetic is plain f64; Ord::max / Ord::min on Epoch: a.max(b) = b < a ? a : b, a.min(b) = b < a ? b : a (on
// equal operands max yields b and min yields a, which only +-0 can tell apart).
// Both distances are evaluated before the test, so max_iterations = 0 evaluates once and returns with iterations = 1. The caller
// bounds max_iterations (2^20): with a precision of 0 or NaN the reference runs until its cap, and this loop must end.
// The one deliberate departure: a NaN difference d. The reference then branches on the sign bit of a NaN, which IEEE leaves to the
// platform; here that is EPH_EVAL_FAILED with failed_at = mid1 and found = 0, before the precision test.
template <class Source, class Target>
__device__ __forceinline__ Separation closest_separation(const Source &src, const Target &tgt, double left, double right,
                                                         double precision, long long max_iterations, int metric) {
    Separation out = {0, 0.0, 0.0, 0, EPH_OK, 0.0};
    double sstart, send, tstart, tend;
    src.bounds(sstart, send);
    tgt.bounds(tstart, tend);
    const double start = tstart < sstart ? sstart : tstart;         // self.trajectory.start().max(reference.start())  :283-288
    const double end = tend < send ? tend : send;                   // self.trajectory.end().min(reference.end())      :291-296
    left = left < start ? start : left;                             // self.start().max(left)   :223
    right = right < end ? right : end;                              // self.end().min(right)    :224
    if (right <= left) return out;                                  // None
    // |at| t1.distance_squared_at(t2, at).unwrap() / t1.distance_at(t2, at).unwrap()
    auto dist = [&](double at, double &d) -> bool {
        V3 a, b;
        if (!src.position(at, a)) return false;                     // self.position(at)?
        if (!tgt.position(at, b)) return false;                     // other.position(at)?
        const V3 r = sub(a, b);
        const double d2 = dot(r, r);
        d = metric ? sqrt(d2) : d2;
        return true;
    };
    long long i = 0;
    double mid1, mid2;
    for (;;) {                                                      // the ternary search
        i += 1;
        out.iterations = (int)i;
        const double total = right - left;
        mid1 = left + total / 3.0;
        mid2 = right - total / 3.0;
        double d1, d2;
        if (!dist(mid1, d1)) { out.status = EPH_EVAL_FAILED; out.failed_at = mid1; return out; }
        if (!dist(mid2, d2)) { out.status = EPH_EVAL_FAILED; out.failed_at = mid2; return out; }
        const double d = d1 - d2;
        if (d != d) { out.status = EPH_EVAL_FAILED; out.failed_at = mid1; return out; }     // the departure told above
        if (fabs(d) < precision || i > max_iterations) break;
        if (!__builtin_signbit(d)) left = mid1; else right = mid2;  // d.is_sign_positive()
    }
    const double time = mid1 + (mid2 - mid1) / 2.0;
    // relative.position(time).unwrap().length(): the reference (the target) first  trajectory.rs:319-325
    V3 tp, sp;
    if (!tgt.position(time, tp) || !src.position(time, sp)) { out.status = EPH_EVAL_FAILED; out.failed_at = time; return out; }
    const V3 r = sub(sp, tp);
    out.found = 1;
    out.time = time;
    out.distance = sqrt(dot(r, r));
    return out;
}

}  // namespace eph
