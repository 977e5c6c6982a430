"""CPU: the restatement of the app's target search (closest_separation_restatement.py) pinned by what the algorithm itself
guarantees, before the GPU tests compare the library with it bit for bit."""
import math

import numpy as np

import closest_separation_restatement as cs


def straight(p0, v, t):
    """a CubicHermiteSpline in uniform straight-line motion: knots p0 + v * t with velocity v"""
    t = np.asarray(t, dtype=np.float64)
    p0, v = np.asarray(p0, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return cs.Hermite(t, p0[None, :] + v[None, :] * t[:, None], np.broadcast_to(v, (len(t), 3)).copy())


A = ([1200.0, -300.0, 50.0], [1.5, 0.25, -0.125])
B = ([-800.0, 2500.0, -400.0], [2.0, -0.5, 0.0625])
TA, TB = np.linspace(0.0, 8192.0, 65), np.linspace(256.0, 8000.0, 122)


def closed_form(a, b):
    """t* of |(pa - pb) + (va - vb) t|: -(dp . dv) / (dv . dv)"""
    dp, dv = np.subtract(a[0], b[0]), np.subtract(a[1], b[1])
    return float(-np.dot(dp, dv) / np.dot(dv, dv))


def test_straight_lines_bracket_the_closed_form_time():
    """two splines in uniform straight-line motion: the squared distance is a parabola, unimodal, so the ternary search never
    discards the minimum: the final bracket contains the closed-form time, and the returned time lies inside the bracket"""
    src, tgt = straight(*A, TA), straight(*B, TB)
    want = closed_form(A, B)
    assert 256.0 < want < 8000.0                                     # inside the common span: an interior minimum
    done = 0
    for metric in (0, 1):
        for left, right in ((-math.inf, math.inf), (0.0, 1e9), (1000.0, 7000.0), (want - 1.0, want + 300.0)):
            for precision in (0.001, 1e-6):
                r = cs.closest_separation(src, tgt, left, right, precision, 1000, metric)
                lo, hi = r["bracket"]
                assert r["found"] and r["status"] == cs.OK and 1 <= r["iterations"] <= 1000, r
                assert lo <= r["time"] <= hi and lo <= want <= hi, (r, want)
                assert max(left, 256.0) <= lo and hi <= min(right, 8000.0)
                p = np.subtract(A[0], B[0]) + np.subtract(A[1], B[1]) * r["time"]
                assert abs(r["distance"] - float(np.linalg.norm(p))) < 1e-6      # the result's distance is the separation at that time
                done += 1
    assert done == 16


def test_iteration_counts_of_small_caps():
    """both distances are evaluated before the test: max_iterations 0, 1, 5 return after 1, 2, 6 iterations"""
    src, tgt = straight(*A, TA), straight(*B, TB)
    for metric in (0, 1):
        for cap, want in ((0, 1), (1, 2), (5, 6)):
            r = cs.closest_separation(src, tgt, -math.inf, math.inf, 0.001, cap, metric)
            assert r["found"] and r["iterations"] == want, (cap, r)
    # the first iteration's answer is the middle of the window
    r = cs.closest_separation(src, tgt, -math.inf, math.inf, 0.001, 0, 0)
    total = 8000.0 - 256.0
    m1, m2 = 256.0 + total / 3.0, 8000.0 - total / 3.0
    assert r["time"] == m1 + (m2 - m1) / 2.0 and r["bracket"] == (256.0, 8000.0)


def test_no_window_is_none():
    """disjoint spans and right <= left: None, without an evaluation"""
    src = straight(*A, TA)
    none = dict(found=False, time=0.0, distance=0.0, iterations=0, status=cs.OK, failed_at=0.0, bracket=None)
    assert cs.closest_separation(src, straight(*B, np.linspace(9000.0, 9900.0, 10)), -math.inf, math.inf) == none
    assert cs.closest_separation(src, straight(*B, np.linspace(8192.0, 9900.0, 10)), -math.inf, math.inf) == none     # touching: right == left
    tgt = straight(*B, TB)
    assert cs.closest_separation(src, tgt, 5000.0, 5000.0) == none
    assert cs.closest_separation(src, tgt, 5000.0, 4000.0) == none
    assert cs.closest_separation(src, tgt, 8000.0, math.inf) == none
    assert cs.closest_separation(src, tgt, -math.inf, 256.0) == none
    assert cs.closest_separation(src, straight(*B, [100.0]), -math.inf, math.inf) == none                            # one knot: start == end


def test_an_empty_target_fails_at_the_first_mid1():
    """an empty spline is bounded by Epoch::MIN / MAX and has no position anywhere: the reference unwraps None at mid1 of the first
    iteration"""
    src = straight(*A, TA)
    empty = cs.Hermite(np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.bounds() == (cs.EPOCH_MIN, cs.EPOCH_MAX)
    for s, t in ((src, empty), (empty, src)):
        r = cs.closest_separation(s, t, -math.inf, math.inf)
        assert not r["found"] and r["status"] == cs.EVAL_FAILED and r["iterations"] == 1
        assert r["failed_at"] == 0.0 + (8192.0 - 0.0) / 3.0 and r["bracket"] == (0.0, 8192.0)
    r = cs.closest_separation(src, empty, 1000.0, 4000.0, metric=1)
    assert r["status"] == cs.EVAL_FAILED and r["failed_at"] == 1000.0 + 3000.0 / 3.0


def test_ord_max_and_min_on_signed_zeros():
    """Ord::max yields the second of equal operands, Ord::min the first"""
    assert math.copysign(1.0, cs.ord_max(0.0, -0.0)) == -1.0 and math.copysign(1.0, cs.ord_max(-0.0, 0.0)) == 1.0
    assert math.copysign(1.0, cs.ord_min(0.0, -0.0)) == 1.0 and math.copysign(1.0, cs.ord_min(-0.0, 0.0)) == -1.0


def test_a_nan_difference_fails_at_mid1():
    """the one deliberate departure from the reference: a NaN difference of the two distances (here inf - inf inside a segment whose
    knots sit at an infinite position) is EVAL_FAILED at mid1, not a branch on the NaN's sign bit"""
    lost = cs.Hermite([0.0, 3000.0], [[math.inf, 0.0, 0.0]] * 2, np.zeros((2, 3)))
    for s, t in ((lost, straight(*A, TA)), (straight(*A, TA), lost)):
        for metric in (0, 1):
            r = cs.closest_separation(s, t, -math.inf, math.inf, metric=metric)
            assert not r["found"] and r["status"] == cs.EVAL_FAILED and r["iterations"] == 1 and r["failed_at"] == 1000.0, r
