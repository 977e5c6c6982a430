"""The restatement of the app's target search, in pure Python floats: RelativeTrajectory::closest_separation_between
(ephemeris/src/trajectory.rs:202-248, window :223-224,283-296) with the two distance closures Trajectory::distance_squared_at /
::distance_at (ephemeris_explorer/src/dynamics/mod.rs:133-146), then PlotSeparation.distance = relative.position(time).unwrap()
.length() (ephemeris_explorer/src/analysis.rs:362-366). Every operation is one IEEE double operation in the reference's order and
association; glam's (a - b).length_squared() is (x*x + y*y) + z*z. Trajectory evaluations are the C oracle's
(orc.Solution.eval(..., with_velocity=False), orc.hermite_eval), the way test_gpu_plot.oracle_plot does it.

Where the reference unwraps a None position the answer is status EVAL_FAILED, failed_at = that epoch, found False. One deliberate
departure, shared with the device code (csrc/trajectory_eval.h): a NaN difference of the two distances -- the reference then
branches on the sign bit of a NaN, which IEEE leaves to the platform -- is EVAL_FAILED with failed_at = mid1, found False."""
import math

import numpy as np

from oracle import orc

EPOCH_MIN, EPOCH_MAX = -1.7976931348623157e308, 1.7976931348623157e308
OK, EVAL_FAILED = 0, 4
APP_PRECISION, APP_MAX_ITERATIONS = 0.001, 1000                     # analysis.rs:346


class Body:
    """a body of an orc.Solution: UniformSpline::{start, end, position}"""

    def __init__(self, osol, body):
        self.osol, self.body = osol, body

    def bounds(self):
        start, interval, npoly = self.osol.info(self.body)
        return start, start + interval * float(npoly)

    def position(self, t):
        p = self.osol.eval(self.body, t, with_velocity=False)
        return None if p is None else (float(p[0]), float(p[1]), float(p[2]))


class Hermite:
    """a CubicHermiteSpline over knot arrays (t[k], pos[k][3], vel[k][3]): ::{start, end, position}; empty: Epoch::MIN / MAX"""

    def __init__(self, t, pos, vel):
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        self.vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)

    def bounds(self):
        return (float(self.t[0]), float(self.t[-1])) if len(self.t) else (EPOCH_MIN, EPOCH_MAX)

    def position(self, t):
        if not len(self.t):
            return None
        r = orc.hermite_eval(self.t, self.pos, self.vel, t)
        return None if r is None else (float(r[0][0]), float(r[0][1]), float(r[0][2]))


def ord_max(a, b):
    """Ord::max: on equal operands (+-0) the second"""
    return a if b < a else b


def ord_min(a, b):
    """Ord::min: on equal operands (+-0) the first"""
    return b if b < a else a


def _answer(found=False, time=0.0, distance=0.0, iterations=0, status=OK, failed_at=0.0, bracket=None):
    return dict(found=found, time=time, distance=distance, iterations=iterations, status=status, failed_at=failed_at, bracket=bracket)


def closest_separation(source, target, left, right, precision=APP_PRECISION, max_iterations=APP_MAX_ITERATIONS, metric=0):
    """-> dict(found, time, distance, iterations, status, failed_at) as the library returns them, plus bracket = the search's
    (left, right) when it returned (None where there was no search)."""
    s0, s1 = source.bounds()
    t0, t1 = target.bounds()
    start, end = ord_max(s0, t0), ord_min(s1, t1)                   # trajectory.rs:283-296
    left, right = ord_max(start, left), ord_min(end, right)         # :223-224
    if right <= left:
        return _answer()

    def distance(at):
        a = source.position(at)                                     # self.position(at)?
        if a is None:
            return None
        b = target.position(at)                                     # other.position(at)?
        if b is None:
            return None
        x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        d2 = (x * x + y * y) + z * z
        return math.sqrt(d2) if metric else d2

    i = 0
    while True:
        i += 1
        total = right - left
        mid1 = left + total / 3.0
        mid2 = right - total / 3.0
        d1 = distance(mid1)
        if d1 is None:
            return _answer(iterations=i, status=EVAL_FAILED, failed_at=mid1, bracket=(left, right))
        d2 = distance(mid2)
        if d2 is None:
            return _answer(iterations=i, status=EVAL_FAILED, failed_at=mid2, bracket=(left, right))
        d = d1 - d2
        if d != d:                                                  # the departure told above
            return _answer(iterations=i, status=EVAL_FAILED, failed_at=mid1, bracket=(left, right))
        if abs(d) < precision or i > max_iterations:
            break
        if math.copysign(1.0, d) > 0.0:                             # d.is_sign_positive()
            left = mid1
        else:
            right = mid2
    time = mid1 + (mid2 - mid1) / 2.0
    tp = target.position(time)                                      # relative.position(time): the reference (the target) first
    sp = source.position(time) if tp is not None else None
    if tp is None or sp is None:
        return _answer(iterations=i, status=EVAL_FAILED, failed_at=time, bracket=(left, right))
    x, y, z = sp[0] - tp[0], sp[1] - tp[1], sp[2] - tp[2]
    return _answer(True, time, math.sqrt((x * x + y * y) + z * z), i, OK, 0.0, (left, right))
