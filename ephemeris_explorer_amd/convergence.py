"""convergence::<M>(problem, h0) of the reference's own integration test, ephemeris/tests/solar_system_convergence.rs:225-285,
on the device: the doubling sweep of step sizes whose answers that test asserts (QuinlanTremaine12 -> 10 min, Stormer13 -> 5 min,
BlanesMoan14A -> 10 min). Every run is a compensated NBodyIntegration (state Double<DVec3>, method "<M><Double>"), as in the test.
At the shipped system's 32 bodies all three answers run as single launches: a run's steady steps are one launch of
k_lm_double_small for the two multistep methods, and the whole run is one launch of k_srkn_double_small for BlanesMoan14A.

The runs of a sweep are independent and their costs halve from one to the next. convergence() takes them one after the other;
convergence_gang() creates the truth run and the next GANG_CANDIDATES candidates together and advances them to the bound in ONE
advance_many -- for a symplectic method at most 32 bodies that is one launch of k_srkn_small_many<Double>, a workgroup per run,
each with its own step count -- and judges the rows in the same order by the same rule: answer, rows and errors are bit for bit
those of convergence()."""
import functools

import numpy as np

STEP_LIMIT = 1 << 40      # "until the bound": advance() stops with BoundReached on the step after the last


class ConvergenceError(Exception):
    """ConvergenceError of the test (:203-207): IntegrationError(StepError) | NoResults | Overstep."""

    def __init__(self, kind, step_error=None):
        self.kind, self.step_error = kind, step_error
        super().__init__(kind if step_error is None else f"{kind}: {step_error}")


def _solve(pos, vel, mu, t0, bound, method, h):
    """Integration::solve with EveryStepSolout (integration/src/lib.rs:506-529): advance until time >= bound.
    -> (end time, y values, dy values)."""
    from . import BOUND_REACHED, NBodyIntegration, StepError
    g = NBodyIntegration(pos, vel, mu, t0, h, method=method, compensated=True)
    g.set_bound(bound)
    try:
        g.advance(STEP_LIMIT)
    except StepError as e:
        if e.status != BOUND_REACHED:
            raise ConvergenceError("IntegrationError", e) from e
    y, dy, end, _ = g.state()
    return end, y, dy


def _solve_many(pos, vel, mu, t0, bound, method, hs):
    """_solve for every h of `hs`, side by side -> one callable per run that returns (end time, y, dy) or raises what _solve
    raises for that run. advance_many reports the first status of the call only: a member's own advance(1) afterwards says what
    stopped it (both stop conditions persist, and that call queues nothing)."""
    from . import BOUND_REACHED, NBodyIntegration, StepError, advance_many
    runs = [NBodyIntegration(pos, vel, mu, t0, h, method=method, compensated=True) for h in hs]
    for g in runs:
        g.set_bound(bound)
    try:
        advance_many(runs, STEP_LIMIT)
    except StepError:
        pass

    def result(g):
        try:
            g.advance(1)
        except StepError as e:
            if e.status != BOUND_REACHED:
                raise ConvergenceError("IntegrationError", e) from e
        y, dy, end, _ = g.state()
        return end, y, dy
    return [functools.partial(result, g) for g in runs]


def _length(d):
    """DVec3::length = dot(self).sqrt(), dot = x*x + y*y + z*z in that order"""
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


GANG_CANDIDATES = 5       # candidates of convergence_gang() that are created and advanced together (the first time: with the truth run)


def _sweep(pos, vel, mu, t0, bound, method, h0, solve_next):
    """the sweep of convergence() on solve_next(h) -> (end time, y, dy) of the run with step h, asked for h0 / 2, h0, 2 h0, ... in
    that order"""
    h = float(h0)
    _, truth_y, truth_dy = solve_next(h / 2.0)
    fmax = functools.partial(functools.reduce, np.fmax)      # f64::max: a NaN operand gives the other one
    rows = []
    while True:
        end, y, dy = solve_next(h)
        ey = float(fmax(_length(y - truth_y) * 1e3, 0.0))
        edy = float(fmax(_length(dy - truth_dy) * 1e3, 0.0))
        if abs(bound - end) != 0.0:
            raise ConvergenceError("Overstep")
        rows.append((h, ey, edy))
        if ey > 10.0 or edy > 1.0:
            break
        h *= 2.0
    if not rows:
        raise ConvergenceError("NoResults")
    return rows[max(len(rows) - 2, 0)][0], np.array(rows)


def convergence(pos, vel, mu, t0, bound, method, h0=75.0):
    """-> (converged h in seconds, rows of (h, largest position error [m], largest velocity error [m/s])).
    The truth run steps with h0 / 2; then h0, 2 h0, 4 h0, ... each to the bound, until the position error against the truth
    exceeds 10 m or the velocity error 1 m/s (positions in km: `length() * 1e3` on the value parts, combined with f64::max).
    The answer is the last h that stayed inside, results[len - 2]. `method` is the base name ("QuinlanTremaine12")."""
    pos, vel, mu = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, mu))
    return _sweep(pos, vel, mu, t0, bound, method, h0, lambda h: _solve(pos, vel, mu, t0, bound, method, h))


def convergence_gang(pos, vel, mu, t0, bound, method, h0=75.0):
    """convergence() with the runs side by side: the truth run and the next GANG_CANDIDATES candidates are created together and
    advanced to the bound in one advance_many; the rows are judged in order by the same rule, and if it has not fired the next
    GANG_CANDIDATES candidates follow the same way. Answer, rows and the three ConvergenceError kinds are those of convergence().
    (The runs of a batch are created together: a run that cannot be CREATED fails the call when its batch begins, where
    convergence() would fail when it reached that run -- or not at all, had the rule fired before it.)"""
    pos, vel, mu = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, mu))
    ready = {}                                               # h -> its run's result, not yet asked for

    def solve_next(h):
        if h not in ready:
            hs = [h]
            while len(hs) < GANG_CANDIDATES + (1 if not ready and h == float(h0) / 2.0 else 0):
                hs.append(hs[-1] * 2.0)
            ready.clear()
            ready.update(zip(hs, _solve_many(pos, vel, mu, t0, bound, method, hs)))
        return ready.pop(h)()
    return _sweep(pos, vel, mu, t0, bound, method, h0, solve_next)
