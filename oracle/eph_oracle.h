/* eph_oracle.h -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * A plain-C restatement of the reference's hot path (Canleskis/ephemeris-explorer, crates `integration`
 * and `ephemeris`, plus the arithmetic the app crate contributes to the path). Every function cites the
 * reference file:line it follows. Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may load this library; the product (ephemeris_explorer_amd/) never does.
 *
 * PARITY PINNING: the reference cannot be built here (no Rust toolchain) and its innermost arithmetic
 * (`particular::gravity::newtonian`, git rev d490707a, Cargo.lock:4277-4285) is not on disk, so the pair
 * formula is "parity unpinned" (orc_set_pair_variant carries the plausible alternatives, the product
 * carries the same four behind -DEPH_PAIR_VARIANT). Everything else is pinned by: the reference's own discrete,
 * integrator-sensitive known answers -- ephemeris/tests/solar_system_convergence.rs:346-357 asserts the converged
 * step of QuinlanTremaine12 / Stormer13 / BlanesMoan14A on its compensated Double<DVec3> state, restated in
 * convergence_double.inc and reproduced (10 / 5 / 10 minutes) by tests/test_convergence_pin.py --, the coefficient
 * tables (tests/golden/coeff_tables.json, generated from the reference's constants), the doc-test known answers
 * (integration/src/lib.rs:32-56,60-93), the spacecraft scenario's assertions
 * (ephemeris/tests/spacecraft_propagation.rs:476-480), an independent Python restatement (oracle/pyoracle.py) and the
 * committed systems fixtures (tests/golden/systems).
 */
#ifndef EPH_ORACLE_H
#define EPH_ORACLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes = integration::StepError (integration/src/lib.rs:312-318) + NBodyPropagatorError::Solout */
enum {
    ORC_OK = 0,
    ORC_STEP_SIZE_UNDERFLOW = 1,
    ORC_MAX_ITERATIONS = 2,
    ORC_BOUND_REACHED = 3,
    ORC_EVAL_FAILED = 4,
    ORC_SOLOUT_EXIT = 5,
    ORC_BAD_ARGUMENT = -1
};

/* ---- Ratio (integration/src/ratio.rs) ---------------------------------------------------------- */
/* from_f64 (:75-103) + normalize (:153-177): out = {numer_hi, numer_lo, denom_hi, denom_lo}; returns the
 * f64 the ratio converts back to (:221-228). */
double orc_ratio_from_f64(double v, int64_t out_nd[4]);
double orc_ratio_to_f64(int64_t n_hi, uint64_t n_lo, int64_t d_hi, uint64_t d_lo);

/* ---- coefficient tables as the f64 the reference multiplies with ------------------------------- */
int orc_srkn_coeffs(const char *name, int *stages, int *fsal, double *A, double *B);
/* w_alpha[j] = (double)(-ALPHA[j+1]), w_beta[j] = (double)BETA_N[j+1], j = 0..order-1;
 * cowell[j] = (double)Cowell<order>::BETA_N[j]; inv_* = 1.0/(double)D */
int orc_elm2_coeffs(const char *name, int *order, double *w_alpha, double *w_beta, double *inv_beta_d,
                    double *cowell, double *inv_cowell_d);
/* A is the flattened strict lower triangle (row s has s entries) */
int orc_erk_coeffs(const char *name, int *stages, int *order, int *order_embedded, int *fsal, double *A,
                   double *B, double *C, double *E);

/* ---- NewtonianGravity::eval (ephemeris/src/propagators/nbody.rs:16-39) --------------------------- */
/* y, ddy: AoS xyz; ddy is ACCUMULATED into (caller zeroes), exactly like the reference. */
/* > 1: gravity evaluated by that many OpenMP threads, partitioned by target body (same bits; all N^2 directed
 * interactions). 0 / 1: the reference's serial pair loop. Process-wide. */
void orc_set_gravity_threads(int threads);
/* tests only: 0 = the pinned pair formula, 1..3 = other plausible evaluation orders of 1/r^3 (sensitivity study) */
void orc_set_pair_variant(int variant);
/* tests only: the device's opt-in EPH_PATH_FAST summation restated -- every target's directed terms c(i, j) chained in source order
 * within S slices of slice_len consecutive sources, the S partial sums then added in slice order (eph_oracle.c gravity_eval_sliced).
 * (0, 0) = off, the default. Process-wide, read at every evaluation: orc_newtonian_gravity_eval and every integrator follow it. */
void orc_set_gravity_slices(int S, int slice_len);
void orc_newtonian_gravity_eval(int n, const double *y, const double *mu, double *ddy);
/* number of (paired) interactions evaluated since process start -- used by bench.py for ns/pair */
uint64_t orc_pair_counter(void);

/* ---- fixed-step N-body integrator (no solout) --------------------------------------------------- */
typedef struct orc_nbody orc_nbody;
/* method: "QuinlanTremaine12" | "Stormer13" (LinearMultistep<_, f64, Substepper<4, BlanesMoan6B>>,
 * integration/src/methods.rs:37-40) or any SRKN table name ("BlanesMoan6B", "BlanesMoan14A", ...)
 * = FixedRungeKutta<SRKN>. h is signed (Backward = negative, propagators/mod.rs:78-82). */
orc_nbody *orc_nbody_new(int n, const double *pos, const double *vel, const double *mu, double t0, double h,
                         const char *method);
orc_nbody *orc_nbody_clone(const orc_nbody *);
void orc_nbody_free(orc_nbody *);
int orc_nbody_advance(orc_nbody *, int64_t nsteps); /* nsteps x Integrator::advance */
void orc_nbody_get_state(const orc_nbody *, double *pos, double *vel, double *t, uint32_t *step_count);
void orc_nbody_get_acc(const orc_nbody *, double *acc); /* current_ddy of the multistep / ddy of SRKN */
void orc_nbody_set_bound(orc_nbody *, double bound);
uint64_t orc_nbody_eval_count(const orc_nbody *);

/* ---- NBodyPropagator + SplineInterpolators solout + UniformSpline ------------------------------ */
typedef struct orc_prop orc_prop;
/* dt > 0; direction +1 Forward / -1 Backward; count[b] = sample_period_b / dt (load/mod.rs:325),
 * degree[b] = LeastSquaresFit.degree */
orc_prop *orc_prop_new(int n, const double *pos, const double *vel, const double *mu, double t0, double dt,
                       int direction, const char *method, const uint32_t *count, const uint32_t *degree);
orc_prop *orc_prop_clone(const orc_prop *);
void orc_prop_free(orc_prop *);
int orc_prop_step(orc_prop *);               /* IncrementalPropagator::step  nbody.rs:200-207 */
int orc_prop_step_n(orc_prop *pr, int64_t n);      /* n steps, stopping at the first error */
int orc_prop_step_to(orc_prop *, double t);  /* ephemeris/src/lib.rs:49-60 */
double orc_prop_time(const orc_prop *);      /* DirectionalPropagator::time  nbody.rs:225-227,502-508 */
int orc_prop_has_reached(const orc_prop *, double t);
double orc_prop_integrator_time(const orc_prop *); /* NBodyPropagator::time nbody.rs:150-152 */
void orc_prop_get_state(const orc_prop *, double *pos, double *vel, double *t, uint32_t *step_count);

typedef struct orc_solution orc_solution;   /* Vec<UniformSpline<DVec3>> */
orc_solution *orc_prop_take_solution(orc_prop *); /* nbody.rs:182-189 */
void orc_solution_free(orc_solution *);
int orc_solution_bodies(const orc_solution *);
/* per body: start [s], interval [s], number of polynomials */
void orc_solution_info(const orc_solution *, int body, double *start, double *interval, int64_t *npoly);
/* copies npoly*8*3 doubles (coeff k of poly p at [(p*8+k)*3 + c], zero padded) and npoly coefficient counts */
void orc_solution_coeffs(const orc_solution *, int body, double *coeffs, int32_t *ncoef);
/* UniformSpline::position / state_vector (trajectory.rs:459-470); returns 1 if `at` is inside, else 0 */
int orc_solution_eval(const orc_solution *, int body, double at, double *pos, double *vel);
/* append b to a (UniformSpline::append / prepend, trajectory.rs:515-539); returns 0 on contiguity failure */
int orc_solution_append(orc_solution *a, const orc_solution *b, int direction);
void orc_solution_clear(orc_solution *so, int body, double at, int after);
orc_solution *orc_solution_clone(const orc_solution *src);
/* Vec<UniformSpline> from its parts, in the layout orc_solution_coeffs returns (polynomials of body 0 first, coefficient k of
 * polynomial p at [(p*8+k)*3 + c]); copies ncoef[p] rows per polynomial and never reads a row at or beyond ncoef[p]. NULL for a
 * negative count or ncoef outside 0..8. */
orc_solution *orc_solution_create(int n, const double *start, const double *interval, const int64_t *npoly, const double *coeffs,
                                  const int32_t *ncoef);

/* LeastSquaresFit::interpolate (ephemeris_explorer/src/dynamics/celestial.rs:24-135):
 * ts[m], xs[m*3] -> coeffs[8*3] (zero padded), returns ncoef after trim, or -1 on Err(()) */
int orc_least_squares_fit(int degree, int m, const double *ts, const double *xs, double *coeffs);
/* Polynomial::eval_and_deriv on one 8x3 coefficient block (trajectory.rs:368-385) */
void orc_poly_eval_and_deriv(int ncoef, const double *coeffs, double tau, double *val, double *deriv);

/* ---- massless path: SpacecraftPropagator<[StateVector;1], ReferenceFrame, Bodies, AdaptiveRungeKutta<ERK>, -----
 * CubicHermiteSplineSolout>  (ephemeris/src/propagators/spacecraft.rs:224-695; integration/src/runge_kutta/
 * explicit.rs:54-141, mod.rs:128-440; ephemeris_explorer/src/dynamics/spacecraft.rs:70-74,218-293,609-641).
 * The bodies are visited in index order (the app's EntityHashMap order is unspecified; the reference test uses an
 * IndexMap in body order, ephemeris/tests/spacecraft_propagation.rs:226-240). */
typedef struct orc_craft orc_craft;
/* eph: the massive bodies' splines (borrowed, must outlive the craft); mu[b]; method: an embedded ERK table name
 * ("Verner87", "DormandPrince54", ...); burns: [start, end), acceleration in the burn frame, ref body index or -1
 * for the inertial frame. */
orc_craft *orc_craft_new(const orc_solution *eph, const double *mu, double t0, const double *pos, const double *vel,
                         const char *method, double h_init, double h_max, double tol_pos, double tol_vel,
                         double fac_min, double fac_max, double fac, uint32_t n_max, int nburns,
                         const double *burn_start, const double *burn_end, const double *burn_acc,
                         const int32_t *burn_ref);
/* the order Bodies::acceleration visits the bodies in (a permutation of 0..n-1; NULL = file order) */
int orc_craft_set_body_order(orc_craft *, const int32_t *order);
void orc_craft_free(orc_craft *);
int orc_craft_step(orc_craft *);              /* IncrementalPropagator::step  spacecraft.rs:598-615 */
int orc_craft_step_to(orc_craft *, double t); /* step_to: until solution.end() >= t */
int64_t orc_craft_knots(const orc_craft *);   /* CubicHermiteSpline points of the current solution */
void orc_craft_get_knots(const orc_craft *, double *t, double *pos, double *vel);
void orc_craft_state(const orc_craft *, double *t, double *pos, double *vel, double *next_h, uint32_t *n_attempts,
                     uint32_t *steps);
uint64_t orc_craft_evals(const orc_craft *);
/* The app's SpacecraftSolout (ephemeris_explorer/src/dynamics/spacecraft.rs:91-162,296-451,514-587): SOI transitions
 * and apsides found on every accepted step. soi_radius[b] per body (INFINITY for the root,
 * load/mod.rs:283-307). Bodies are visited in body order (the reference iterates an EntityHashMap). Call right
 * after orc_craft_new. apsis kind: 0 = Periapsis, 1 = Apoapsis. Getters return the count (arrays may be NULL). */
void orc_craft_enable_events(orc_craft *, const double *soi_radius);
int64_t orc_craft_transitions(const orc_craft *, double *time, int32_t *body);
int64_t orc_craft_apsides(const orc_craft *, double *time, double *distance, int32_t *body, int32_t *kind);
/* CubicHermiteSpline::state_vector (trajectory.rs:766-797): returns 0 for None */
int orc_hermite_eval(int64_t nknots, const double *t, const double *pos, const double *vel, double at, double *p,
                     double *v);
/* generic scalar first-order problem y' = lambda*y for the doc-test known answers (integration/src/lib.rs:32-93):
 * fixed-step ERK (method, h) or adaptive (h_init, h_max, atol, rtol like the doc-test's tolerance closure);
 * returns y(t_end) */
/* the controller's powf: 0 = correctly rounded double-double evaluation (default, the pinned definition),
 * 1 = this host's libm pow (what the Rust reference would call here) */
void orc_set_pow_mode(int mode);
double orc_cr_pow(double x, double y);
double orc_doc_test_decay(const char *method, int adaptive, double h, double h_max, double atol, double rtol,
                          double t_end, uint32_t *steps);

/* ---- the reference's convergence test on Double<DVec3> (ephemeris/tests/solar_system_convergence.rs) ---- */
/* Integration::solve of the generic steppers on the compensated variable type of :12-110; out_y / out_dy hold
 * (value, error) per component: [n][3][2]. max_steps <= 0: run to the bound. Returns the StepError status. */
int orc_double_solve(int n, const double *pos, const double *vel, const double *mu, double t0, double bound, double h,
                     const char *method, int64_t max_steps, double *out_y, double *out_dy, double *end_time);
/* convergence::<M>(problem, h0) :218-296: the largest h of the doubling sweep whose 1-year error vs the h0/2 run
 * stays within 10 m / 1 m/s. rows: max_rows x {h [s], position error [m], velocity error [m/s]}. */
double orc_convergence(int n, const double *pos, const double *vel, const double *mu, double t0, double bound,
                       const char *method, double h0, int max_rows, double *rows, int *nrows, int *status);

#ifdef __cplusplus
}
#endif
#endif
