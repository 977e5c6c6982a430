// double_state.h -- the compensated variable type of the reference's own convergence test, Double<DVec3>
// (ephemeris/tests/solar_system_convergence.rs:12-110), and the stepper formulas on it, stated once for every kernel that
// integrates a `<Double>` handle (step_double_small.hip, double_step.hip).
//
// DVec3 is component-wise for every operator the steppers use, so the device type is one (value, error) pair per component.
// Every operator below is the reference's operator of the same name, operation for operation; the forms depend on the build's
// -ffp-contract=off -fno-fast-math (an optimiser allowed to reassociate would cancel every error term to zero).
//
// The acceleration has no error part in the reference either: NewtonianGravity::eval (:117-140) fills ddy with
// Double::new(ZERO) and accumulates into `.value`, so `ddy` is Double{value, error: +0.0} wherever a stepper reads it. The
// literal +0.0 goes through the same operators here (0.0 * w is -0.0 for a negative weight, and -0.0 + -0.0 stays -0.0 where
// +0.0 would not): nothing is dropped by hand.
#pragma once
#include <hip/hip_runtime.h>

#include "eph_internal.h"

namespace eph {

struct Dbl { double value, error; };

// ---- kernel argument blocks of the `<Double>` kernels (LmArgs is taken by value by the plain kernels and stays as it is) -------
struct LmDoubleArgs {
    LmArgs a;                  // the plain handle's arguments: Y / V hold the VALUE parts, A the accelerations
    double *YE, *VE;           // error parts: y ring [L][3][npad] (same slots as Y), current velocity [3][npad]
    int do_cowell;             // per-step kernel: form the velocity of level a.cur (its acceleration is in the ring)
};
struct KickDriftDouble { const double *acc; double *v, *ve, *y, *ye; double hb, ha; Body4 *pos_out; };

__host__ __device__ __forceinline__ Dbl two_sum(double a, double b) {            // :30-40
    const double value = a + b;
    const double v = value - a;
    const double error = (a - (value - v)) + (b - v);
    return Dbl{value, error};
}
__host__ __device__ __forceinline__ Dbl fast_two_sum(double a, double b) {       // :50-59
    const double value = a + b;
    const double error = b - (value - a);
    return Dbl{value, error};
}
__host__ __device__ __forceinline__ Dbl dbl_add(Dbl s, Dbl o) {                  // impl Add :62-73
    const Dbl sum = two_sum(s.value, o.value);
    return fast_two_sum(sum.value, (sum.error + s.error) + o.error);
}
__host__ __device__ __forceinline__ Dbl dbl_sub(Dbl s, Dbl o) {                  // impl Sub :75-86; two_sub = two_sum(a, -b) :42-48
    const Dbl sum = two_sum(s.value, -o.value);
    return fast_two_sum(sum.value, (sum.error + s.error) - o.error);
}
__host__ __device__ __forceinline__ Dbl dbl_mul(Dbl s, double r) { return Dbl{s.value * r, s.error * r}; }   // :88-98
__host__ __device__ __forceinline__ Dbl dbl_div(Dbl s, double r) { return Dbl{s.value / r, s.error / r}; }   // :100-110
// an acceleration as the steppers see it: Double{value, error: +0.0}
__host__ __device__ __forceinline__ Dbl dbl_acc(double a) { return Dbl{a, 0.0}; }

// ------------------------------------------------------------------------------------------------------
// ELM2::advance and Cowell::update_velocity on Double (second_order/mod.rs:93-121, cowell.rs:19-53), the forms of
// force_common.h's lm_predict / lm_cowell: yv[j] / ye[j] / av[j] = value, error and acceleration of level (newest - j).
// ------------------------------------------------------------------------------------------------------
// sum1 alone: it needs positions only, so the single-workgroup kernel runs it beside the pair arithmetic
template <int L>
__device__ __forceinline__ Dbl lm_sum1_double(const double (&yv)[L], const double (&ye)[L], const double *wa) {
    Dbl s1{0.0, 0.0};                                    // State::zero -> Default
#pragma unroll
    for (int j = 0; j < L; ++j) s1 = dbl_add(s1, dbl_mul(Dbl{yv[j], ye[j]}, wa[j]));   // *sum1 = *sum1 + *y * (1.0 * -ALPHA[j+1])
    return s1;
}
template <int L>
__device__ __forceinline__ Dbl lm_sum2_double(const double (&av)[L], const double *wb) {
    Dbl s2{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < L; ++j) s2 = dbl_add(s2, dbl_mul(dbl_acc(av[j]), wb[j]));      // *sum2 = *sum2 + *ddy * (1.0 * BETA_N[j+1])
    return s2;
}
template <int L>
__device__ __forceinline__ Dbl lm_predict_double(const double (&yv)[L], const double (&ye)[L], const double (&av)[L],
                                                 const double *wa, const double *wb, double hh) {
    const Dbl s1 = lm_sum1_double<L>(yv, ye, wa), s2 = lm_sum2_double<L>(av, wb);
    return dbl_add(s1, dbl_mul(s2, hh));                 // *y = *sum1 + *sum2 * (h * h * Ratio::from_recip(BETA_D))
}
// av[0] = acceleration of the new level, av[j] the levels before it; y_new / y_prev the new level and the one before
template <int L>
__device__ __forceinline__ Dbl lm_cowell_double(const double (&av)[L], Dbl y_new, Dbl y_prev, const double *cw, double h,
                                                double hc) {
    Dbl s{0.0, 0.0};
#pragma unroll
    for (int j = 0; j < L; ++j) s = dbl_add(s, dbl_mul(dbl_acc(av[j]), cw[j]));
    return dbl_add(dbl_div(dbl_sub(y_new, y_prev), h), dbl_mul(s, hc));   // *dy = (*y - *ym1) / h + *work * (h * 1/BETA_D)
}

// SRKN stage update of one (body, component) behind its force evaluation   symplectic.rs:90-97
__device__ __forceinline__ void kick_drift_double(const KickDriftDouble &kd, size_t o, int body, int comp) {
    const Dbl vn = dbl_add(Dbl{kd.v[o], kd.ve[o]}, dbl_mul(dbl_acc(kd.acc[o]), kd.hb));   // *dy = *dy + *ddy * (h * C::B[s])
    kd.v[o] = vn.value;
    kd.ve[o] = vn.error;
    const Dbl yn = dbl_add(Dbl{kd.y[o], kd.ye[o]}, dbl_mul(vn, kd.ha));                   // *y = *y + *dy * (h * C::A[s])
    kd.y[o] = yn.value;
    kd.ye[o] = yn.error;
    reinterpret_cast<double *>(kd.pos_out + body)[comp] = yn.value;                       // the force reads `.value`
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// double_step.hip (compiled once): the per-step forms, any n
int launch_lm_double_step(hipStream_t s, const LmDoubleArgs &d);     // [Cowell of level a.cur] + [predictor of the next level, a.do_predict]
int launch_kick_drift_double(hipStream_t s, int n, int npad, const KickDriftDouble &kd);
// (the single-workgroup form, step_double_small.hip, exists once per evaluation order: launch_lm_double_small, eph_internal.h)

}  // namespace eph
