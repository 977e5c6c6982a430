"""convergence::<M>(problem, h0) of the reference's own integration test, ephemeris/tests/solar_system_convergence.rs:225-285,
on the device: the doubling sweep of step sizes whose answers that test asserts (QuinlanTremaine12 -> 10 min, Stormer13 -> 5 min,
BlanesMoan14A -> 10 min). Every run is a compensated NBodyIntegration (state Double<DVec3>, method "<M><Double>"), as in the test.
At the shipped system's 32 bodies all three answers run as single launches: a run's steady steps are one launch of
k_lm_double_small for the two multistep methods, and the whole run is one launch of k_srkn_double_small for BlanesMoan14A."""
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


def _length(d):
    """DVec3::length = dot(self).sqrt(), dot = x*x + y*y + z*z in that order"""
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def convergence(pos, vel, mu, t0, bound, method, h0=75.0):
    """-> (converged h in seconds, rows of (h, largest position error [m], largest velocity error [m/s])).
    The truth run steps with h0 / 2; then h0, 2 h0, 4 h0, ... each to the bound, until the position error against the truth
    exceeds 10 m or the velocity error 1 m/s (positions in km: `length() * 1e3` on the value parts, combined with f64::max).
    The answer is the last h that stayed inside, results[len - 2]. `method` is the base name ("QuinlanTremaine12")."""
    pos, vel, mu = (np.ascontiguousarray(a, dtype=np.float64) for a in (pos, vel, mu))
    h = float(h0)
    _, truth_y, truth_dy = _solve(pos, vel, mu, t0, bound, method, h / 2.0)
    fmax = functools.partial(functools.reduce, np.fmax)      # f64::max: a NaN operand gives the other one
    rows = []
    while True:
        end, y, dy = _solve(pos, vel, mu, t0, bound, method, h)
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
