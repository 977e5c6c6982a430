"""Synthetic body tables with PLANTED epochs, and the scenarios that walk spacecraft onto them: shared by tests/test_synthetic_tables.py
(CPU: the C oracle against the Python restatement) and tests/test_gpu_craft_lookup.py (device against the C oracle). A plain module, no
fixtures.

Why: the lookup of a massive body's polynomial (UniformSpline::get_polynomial + Horner, trajectory.rs:398-410,551-617) is stated three
times for the device -- spline_locate, spline_locate_fast (csrc/craft_device.h) and the speculative locate_spec (csrc/craft_sweep.hip) --
and reaches the sweep kernels through four terms (bodies_acceleration, body_term, body_term_cached, body_term_wave) plus
spline_state_vector (trajectory_eval.h), all promised to give the reference's bits. Tables fitted by the N-body propagator never put a stage epoch on a polynomial boundary except by accident, never
fail entry_fast, agree at their boundaries to round-off and start every body at one epoch. These tables do the opposite on purpose.

The tables (make_body): every body moves on a circle; polynomial p holds the Taylor rows of that motion about its own start, truncated to
the polynomial's row count, so the pieces are smooth enough for the step-size controller and differ at their boundaries by the truncation.
  * row counts run through 0..8 within one table (eph_solution_create accepts ncoef = 0: some polynomials of body 1, the light one, have no rows);
  * the `jumps` body (always the body the craft orbit) carries in addition a position and a velocity offset of alternating sign per
    polynomial (2^-7 .. 2^-9 km, ~10^9 ulps): the neighbouring polynomial evaluated at a boundary gives grossly different bits;
  * z rows of odd degree are -0.0 (the motion is planar), and every fifth polynomial of three or more rows ends in a row of -0.0: the
    first Horner step `0.0 + c` of horner_row and the zero padding behind ncoef both meet signed zeros.
NaN epochs are out of scope (the C oracle's ceil -> uint64_t cast is undefined there); no scenario has one.

Scenario -> the kernel arm it is there for
  A  boundary walk: 70 craft (a full wave and a partial one in the thread-per-craft forms) take 16 steps of exactly 64 s from t0 == start
     of bodies 0 and 1 to start + span of bodies 0 and 2, a knot on every boundary of the 64 s body, then EvalFailed. local == +0 (the
     folded sign test of locate_spec sends `t == start` to body_position_generic in bodies_acceleration, and through body_term_wave's
     mask to body_term_cached, i.e. spline_locate_fast),
     local == k * interval exactly (ceil - 1, not floor: tau == 1 of polynomial k - 1), local == span (idx == npoly - 1, not npoly).
  B  one ulp around: craft started at nextafter(boundary, +-inf), nextafter(start, -inf) (fails before any attempt), start, start + span,
     nextafter(start + span, +inf) of a dyadic table; then t0 = start + interval * k on a table whose intervals are the committed systems'
     own 8 * dt * count. With the committed (integer) epochs start + interval * k, the difference back and its quotient are all exact, so
     that table starts at 2^60 s, where the spacing of doubles (256 s) does not divide the intervals: for three k in four local / interval
     is not the integer k and ceil decides the side (B_LIVENESS_K checks that in numpy). div_refined against the IEEE quotient at the
     numerators nearest an integer quotient.
  C  drifted lanes: 136 craft from a low orbit out to 50 radii against 32 s polynomials, advanced with step_n: the lanes of one wave end up
     hundreds of polynomials apart. horner_lane_rows in the undealt static form (the prefetched row belongs to the first lane only), the
     per-lane reload (load_row) of body_term_wave / body_term_cached (idx != lb.idx) in the wave form, the queue form's refill.
  D  mixed entries and body counts: one body whose interval is 2^210 s (one polynomial; k_body_reciprocals leaves rinv == +0.0, entry_fast
     fails: the `all_good == false` arm, i0 masked to row 0, body_position_generic; in the wave form the lane's entry_fast ballot sends
     the wave to body_term_cached, whose spline_locate_fast divides with the compiler's division) placed first, in the middle and last, which toggles
     all_good from body to body; tables of 1, 2, 64 and 65 bodies (the pipeline's prologue and discarded last lookup; k_craft_wave through
     body_term in two chunks above 64); one case under set_body_order with a TNB burn whose reference body is not at its own index in the
     visiting order (bodies_by_index != bodies).
  E  a lane falls off: bodies end at different epochs, 72 craft of different step sizes run past the shortest body's end: a failing lane
     stays in the ballots and must not disturb its neighbours; at least three different step counts among the failing craft and a failure
     inside a middle stage (failed_stage).
  F  burn on a boundary: a TNB burn relative to the jumps body from t == start (tau == 0) to a polynomial boundary, and a second one from
     boundary to boundary: the craft steps onto the segment bounds exactly, so spline_locate / spline_state_vector (burn_acceleration) see
     tau == 0 and tau == 1.
Every scenario runs on Verner87, DormandPrince54 (FSAL) and Fine45 (Nystroem); A also on Verner98 (16 stages) and on pair variant 4."""
import math

import numpy as np

MU0, MU1, MU2 = 398600.4418, 4902.800066, 1.32712440018e11
EVAL_FAILED = 4
INF = 1.7976931348623157e308
METHODS = ("Verner87", "DormandPrince54", "Fine45")
# (radius [km], angular rate [rad/s], phase) of the three ordinary bodies' circles
ORBITS = ((1000.0, 1.0e-4, 0.3), (384400.0, 2.66e-6, 1.0), (1.496e8, 1.99e-7, 2.0))
JUMP_POS = np.array([2.0 ** -7, -2.0 ** -8, 2.0 ** -9])
JUMP_VEL = np.array([-2.0 ** -9, 2.0 ** -8, 2.0 ** -9])


def circle(orbit, tau):
    """(position, velocity) on the circle at tau seconds after the table's origin of time"""
    r, w, ph = orbit
    a = ph + w * tau
    return np.array([r * math.cos(a), r * math.sin(a), 0.0]), np.array([-r * w * math.sin(a), r * w * math.cos(a), 0.0])


def make_body(orbit, interval, npoly, counts, first_tau=0.0, jumps=False):
    """npoly polynomials of `interval` seconds; polynomial p starts first_tau + interval * p after the table's origin of time and has
    counts[p % len(counts)] rows: the Taylor rows of the circle about its start, in tau = (t - start_p) / interval"""
    r, w, ph = orbit
    out = []
    for p in range(npoly):
        n = counts[p % len(counts)]
        a = ph + w * (first_tau + interval * p)
        rows = np.zeros((n, 3))
        for k in range(n):
            s = r * (w * interval) ** k / math.factorial(k)
            rows[k] = [s * math.cos(a + k * math.pi / 2.0), s * math.sin(a + k * math.pi / 2.0), -0.0 if k % 2 else 0.0]
        if jumps:
            sign = 1.0 if p % 2 else -1.0
            if n >= 1:
                rows[0] += sign * JUMP_POS
            if n >= 2:
                rows[1] += sign * JUMP_VEL
        if n >= 3 and p % 5 == 3:
            rows[n - 1] = -0.0
        out.append(rows)
    return out


def constant_body(j):
    """light, far and at rest: (start, interval, polys, mu), one polynomial of one row; the starts differ from body to body"""
    a = 0.7 * j
    return 4000.0 - j, 2048.0, [np.array([[1.0e6 * math.cos(a), 1.0e6 * math.sin(a), 3.0e5 + j]])], 1.0e-3 * (j + 1)


def huge_body():
    """interval 2^210 s: outside the guarded range of the shared-reciprocal division, rinv == +0.0 in the device table"""
    rows = np.array([[5.0e6, -4.0e6, 3.0e6], [1.0e5, 2.0e5, -0.0], [7.0, -0.0, 9.0], [1.0, 2.0, 3.0], [-0.0, 0.5, 0.25], [0.125, -0.0, 1.0],
                     [3.0, 2.0, 1.0], [-0.0, -0.0, 2.0]])
    return 0.0, 2.0 ** 210, [rows], 10.0


def orbiting(tau, radii, tilt=0.1):
    """circular orbits of the given radii about body 0 where it is tau after the origin of time -> pos[n][3], vel[n][3]"""
    bp, bv = circle(ORBITS[0], tau)
    pos, vel = [], []
    for i, r in enumerate(radii):
        a = 0.37 * i
        u = np.array([math.cos(a), math.sin(a), tilt])
        u /= np.linalg.norm(u)
        w = np.cross([0.0, 0.0, 1.0], u)
        w /= np.linalg.norm(w)
        pos.append(bp + r * u)
        vel.append(bv + math.sqrt(MU0 / r) * w)
    return np.array(pos), np.array(vel)


class Scenario:
    """One table, one batch, one call sequence. table = (start[nb], interval[nb], polys[nb]); t0 scalar or per craft; params = the
    AdaptiveMethodParams as a dict (h_init, h_max, tol_pos, tol_vel); burns[craft] = [(start, end, acc, ref)]; calls = [("propagate", t) |
    ("step_n", k)]; liveness(scenario, method, results) asserts on the ORACLE's results (run_oracle) that the scenario steps on what it was
    planted for; py_craft = the craft the (slow) Python restatement runs as well."""

    def __init__(self, name, table, mu, t0, pos, vel, params, calls, liveness, burns=None, body_order=None, py_craft=None, max_knots=96,
                 methods=METHODS):
        self.name, self.table, self.mu = name, table, np.asarray(mu, dtype=np.float64)
        self.pos, self.vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
        self.n = len(self.pos)
        self.t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(t0, dtype=np.float64), (self.n,)))
        self.params = dict(h_init=60.0, h_max=INF, tol_pos=1e-3, tol_vel=1e-3)
        self.params.update(params)
        self.calls, self.liveness = calls, liveness
        self.burns = burns if burns is not None else [[] for _ in range(self.n)]
        self.body_order = body_order
        self.py_craft = list(range(self.n)) if py_craft is None else list(py_craft)
        self.max_knots, self.methods = max_knots, methods

    @property
    def n_bodies(self):
        return len(self.mu)


def python_table(table):
    """the table as oracle/pyoracle.py takes it"""
    from oracle import pyoracle as po
    return [{"start": float(s), "interval": float(iv), "polys": [[po.Vec(*row) for row in poly] for poly in polys]}
            for s, iv, polys in zip(*table)]


def run_oracle(sc, method, solution):
    """the scenario on orc.Craft over `solution` (orc.Solution.from_parts(*sc.table)) -> per craft dict(status, craft): step_to / step
    until the first error, after which the craft is left alone, like a failed craft of a device batch"""
    from oracle import orc
    p = sc.params
    out = []
    for i in range(sc.n):
        c = orc.Craft(solution, sc.mu, sc.t0[i], sc.pos[i], sc.vel[i], method, h_init=p["h_init"], h_max=p["h_max"], tol_pos=p["tol_pos"],
                      tol_vel=p["tol_vel"], burns=sc.burns[i], body_order=sc.body_order)
        out.append(dict(status=_run_calls(sc, c.step_to, c.step), craft=c))
    return out


def _run_calls(sc, step_to, step):
    st = 0
    for what, arg in sc.calls:
        if st:
            break
        if what == "propagate":
            st = step_to(arg)
        else:
            for _ in range(arg):
                st = step()
                if st:
                    break
    return st


def run_python(sc, method, i, table=None):
    """craft i of the scenario on pyoracle.Craft -> (status, craft)"""
    from oracle import pyoracle as po
    p = sc.params
    c = po.Craft(table if table is not None else python_table(sc.table), sc.mu, float(sc.t0[i]), sc.pos[i], sc.vel[i], method, p["tol_pos"],
                 sc.burns[i], h_init=p["h_init"], body_order=sc.body_order)
    c.h_max, c.tol_pos, c.tol_vel = p["h_max"], p["tol_pos"], p["tol_vel"]

    def step_to(t):
        while not c.knots[-1][0] >= t:
            st = c.step()
            if st:
                return st
        return 0
    return _run_calls(sc, step_to, c.step), c


def nodes(method):
    """the stage nodes c_i of the pair"""
    from oracle import pyoracle as po
    return [po._ratio(r) for r in po.tables()["methods"][method]["C"]["ratio"]]


def failed_stage(method, t, h, end):
    """the first stage of the attempt (t, h) whose epoch lies beyond `end`, or None"""
    for s, c in enumerate(nodes(method)):
        if t + h * c > end:
            return s
    return None


def body_end(sc, b):
    s, iv, polys = sc.table[0][b], sc.table[1][b], sc.table[2][b]
    return s + iv * float(len(polys))


# ---- A ----------------------------------------------------------------------------------------------------------------------------
def _table_abc(start0=4096.0, n0=16, n1=10, n2=5):
    """intervals 64, 128 and 256 s; starts start0, start0 and start0 - 256; body 0 jumps"""
    return ([start0, start0, start0 - 256.0], [64.0, 128.0, 256.0],
            [make_body(ORBITS[0], 64.0, n0, [1, 2, 3], jumps=True), make_body(ORBITS[1], 128.0, n1, [4, 5, 0, 6, 7]),
             make_body(ORBITS[2], 256.0, n2, [8, 7, 8], first_tau=-256.0)])


def _live_a(sc, method, res):
    want = 4096.0 + 64.0 * np.arange(17)
    assert body_end(sc, 0) == body_end(sc, 2) == want[-1] and sc.table[0][0] == sc.table[0][1] == want[0]
    for i, r in enumerate(res):
        kt = r["craft"].knots()[0]
        assert r["status"] == EVAL_FAILED, (sc.name, method, i, r["status"])
        assert len(kt) == 17 and np.array_equal(kt, want), (sc.name, method, i, kt)
        # the first stage of step 1 was at local == +0 of bodies 0 and 1; the first stage of the failing attempt (and the last of step 16,
        # whose node is 1) at local == span of bodies 0 and 2
        assert kt[0] - sc.table[0][0] == 0.0 and not np.signbit(kt[0] - sc.table[0][0])
        assert kt[-1] - sc.table[0][0] == 64.0 * 16.0 and r["craft"].state()["attempts"] == 16


def scenario_a():
    pos, vel = orbiting(0.0, 7000.0 + 3.0 * np.arange(70))
    return Scenario("A", _table_abc(), [MU0, MU1, MU2], 4096.0, pos, vel, dict(h_init=64.0, h_max=64.0, tol_pos=1e3, tol_vel=1e3),
                    [("propagate", 6000.0)], _live_a, py_craft=[0, 33, 63, 64, 69], methods=METHODS + ("Verner98",))


# ---- B ----------------------------------------------------------------------------------------------------------------------------
def _live_b_dyadic(sc, method, res):
    fails = {6: 0, 8: 0, 9: 0}                       # nextafter(start, -inf), start + span, nextafter(start + span, +inf)
    for i, r in enumerate(res):
        st = r["craft"].state()
        if i in fails:
            assert r["status"] == EVAL_FAILED and st["attempts"] == 0 and len(r["craft"].knots()[0]) == 1, (sc.name, method, i)
        else:
            assert r["status"] == 0 and st["steps"] == 3, (sc.name, method, i, r["status"])


def scenario_b_dyadic():
    table = _table_abc(n0=8, n1=5, n2=4)          # ends: 4608, 4736, 4864
    start, end = 4096.0, 4608.0
    t0 = []
    for b in (start + 64.0, start + 128.0, start + 320.0):
        t0 += [np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
    t0 += [np.nextafter(start, -np.inf), start, end, np.nextafter(end, np.inf)]
    t0 = np.array(t0)
    pos, vel = [], []
    for i, t in enumerate(t0):
        p, v = orbiting(t - start, [7000.0 + 100.0 * i])
        pos.append(p[0]), vel.append(v[0])
    return Scenario("B-dyadic", table, [MU0, MU1, MU2], t0, pos, vel, dict(h_init=16.0, h_max=16.0, tol_pos=1e3, tol_vel=1e3),
                    [("step_n", 1), ("step_n", 2)], _live_b_dyadic)


B_START = 2.0 ** 60
B_INTERVALS = (4800.0, 14400.0, 33600.0)          # 8 * dt * count of three bodies of tests/golden/systems/full_solar_system_2433282.5
B_LIVENESS_K = np.arange(1.0, 25.0)


def _live_b_inexact(sc, method, res):
    from conftest import load_system
    s = load_system("full_solar_system_2433282.5")
    committed = set((s.dt * s.count.astype(np.float64) * 8.0).tolist())
    assert set(B_INTERVALS) <= committed
    t0 = B_START + B_INTERVALS[0] * B_LIVENESS_K                              # binary64, as the scenario forms it
    assert np.array_equal(t0, sc.t0)
    q = (t0 - B_START) / B_INTERVALS[0]
    assert np.count_nonzero(q != B_LIVENESS_K) * 4 >= len(B_LIVENESS_K), q
    assert np.count_nonzero(np.ceil(q) != B_LIVENESS_K) >= 4 and np.count_nonzero(np.ceil(q) == B_LIVENESS_K) >= 4     # both sides occur
    for i, r in enumerate(res):
        assert r["status"] == 0 and r["craft"].state()["steps"] == 2, (sc.name, method, i, r["status"])


def scenario_b_inexact():
    iv = B_INTERVALS
    table = ([B_START] * 3, list(iv), [make_body(ORBITS[0], iv[0], 26, [1, 2, 3, 4, 5, 6, 7, 8], jumps=True),
                                       make_body(ORBITS[1], iv[1], 9, [4, 5, 0, 6, 7]), make_body(ORBITS[2], iv[2], 4, [8, 7])])
    t0 = B_START + iv[0] * B_LIVENESS_K
    pos, vel = [], []
    for i, k in enumerate(B_LIVENESS_K):
        p, v = orbiting(iv[0] * k, [42000.0 + 50.0 * i])
        pos.append(p[0]), vel.append(v[0])
    return Scenario("B-inexact", table, [MU0, MU1, MU2], t0, pos, vel, dict(h_init=1024.0, h_max=1024.0, tol_pos=1e3, tol_vel=1e3),
                    [("step_n", 2)], _live_b_inexact, py_craft=range(0, 24, 3))


# ---- C ----------------------------------------------------------------------------------------------------------------------------
def polynomial_of(sc, b, t):
    """index of body b's polynomial at t, the reference's way (ceil - 1)"""
    local = t - sc.table[0][b]
    return max(int(math.ceil(local / sc.table[1][b])) - 1, 0)


def _live_c(sc, method, res):
    for i, r in enumerate(res):
        assert r["status"] == 0 and r["craft"].state()["steps"] == 40, (sc.name, method, i, r["status"])
    where = {polynomial_of(sc, 0, r["craft"].state()["t"]) for r in res[:64]}
    assert len(where) >= 8, (sc.name, method, sorted(where))


def scenario_c():
    n = 2600                                       # 83 200 s: 40 steps of at most 2048 s
    table = ([0.0, 0.0, 0.0], [32.0, 32.0, 32.0], [make_body(ORBITS[0], 32.0, n, [1, 2, 3, 4, 5, 6, 7, 8], jumps=True),
                                                   make_body(ORBITS[1], 32.0, n, [4, 5, 0, 6, 7]), make_body(ORBITS[2], 32.0, n, [8, 7])])
    pos, vel = orbiting(0.0, 6600.0 * (1.0 + 49.0 * np.arange(136) / 135.0))
    return Scenario("C", table, [MU0, MU1, MU2], 0.0, pos, vel, dict(h_init=30.0, h_max=2048.0, tol_pos=1e-2, tol_vel=1e-2),
                    [("step_n", 1), ("step_n", 7), ("step_n", 32)], _live_c, py_craft=[0, 1, 63, 64, 127, 128, 135])


# ---- D ----------------------------------------------------------------------------------------------------------------------------
def _live_ok(sc, method, res):
    for i, r in enumerate(res):
        assert r["status"] == 0, (sc.name, method, i, r["status"])
        assert len(r["craft"].knots()[0]) >= 12


def _assemble(names):
    """a table from 'a' / 'b' / 'c' (the three ordinary bodies, 64 / 128 / 256 s), 'H' (the 2^210 s body) and integers (constants)"""
    base = _table_abc(n0=20, n1=10, n2=6)          # every one ends at 5376
    mus = {"a": MU0, "b": MU1, "c": MU2}
    start, interval, polys, mu = [], [], [], []
    for nm in names:
        if nm in mus:
            k = "abc".index(nm)
            s, iv, pl, m = base[0][k], base[1][k], base[2][k], mus[nm]
        elif nm == "H":
            s, iv, pl, m = huge_body()
        else:
            s, iv, pl, m = constant_body(nm)
        start.append(s), interval.append(iv), polys.append(pl), mu.append(m)
    return (start, interval, polys), mu


def scenarios_d():
    pos, vel = orbiting(0.0, 7000.0 + 500.0 * np.arange(6))
    par = dict(h_init=50.0, h_max=64.0, tol_pos=1e3, tol_vel=1e3)
    calls = [("propagate", 4096.0 + 1000.0)]
    out = []
    layouts = {"D-huge-first": ["H", "a", "b", "c"], "D-huge-middle": ["a", "H", "b", "c"], "D-huge-last": ["a", "b", "c", "H"],
               "D-1": ["a"], "D-2": ["a", "H"],
               "D-64": ["a", "b", "c"] + list(range(37)) + ["H"] + list(range(37, 60)),
               "D-65": ["a", "b", "c"] + list(range(37)) + ["H"] + list(range(37, 61))}
    for name, names in layouts.items():
        table, mu = _assemble(names)
        assert len(mu) == {"D-1": 1, "D-2": 2, "D-64": 64, "D-65": 65}.get(name, 4)
        out.append(Scenario(name, table, mu, 4096.0, pos, vel, par, calls, _live_ok, py_craft=[0, 5] if len(mu) < 64 else [5]))
    # the visiting order a permutation, and a TNB burn about body 0, which the order visits second
    table, mu = _assemble(["a", "H", "b", "c", 3])
    burns = [[(4096.0 + 100.0, 4096.0 + 300.0, [2e-4, 1e-4, -5e-5], 0)] for _ in range(6)]
    order = [2, 0, 4, 1, 3]
    assert order.index(0) != 0
    out.append(Scenario("D-order", table, mu, 4096.0, pos, vel, par, calls, _live_ok, burns=burns, body_order=order, py_craft=[0, 5]))
    return out


# ---- E ----------------------------------------------------------------------------------------------------------------------------
def _live_e(sc, method, res):
    end = min(body_end(sc, b) for b in range(sc.n_bodies))
    assert end == body_end(sc, 0) and len({body_end(sc, b) for b in range(sc.n_bodies)}) == sc.n_bodies
    steps, stages = set(), set()
    last = len(nodes(method)) - 1
    for i, r in enumerate(res):
        assert r["status"] == EVAL_FAILED, (sc.name, method, i, r["status"])
        st = r["craft"].state()
        steps.add(st["steps"])
        stages.add(failed_stage(method, st["t"], st["next_h"], end))
    assert len(steps) >= 3, (sc.name, method, steps)
    assert any(s is not None and 0 < s < last for s in stages), (sc.name, method, stages)


def scenario_e():
    table = ([0.0, 0.0, 0.0], [32.0, 128.0, 256.0], [make_body(ORBITS[0], 32.0, 40, [1, 2, 3, 4, 5, 6, 7, 8], jumps=True),
                                                     make_body(ORBITS[1], 128.0, 16, [4, 5, 0, 6, 7]), make_body(ORBITS[2], 256.0, 10, [8, 7])])
    pos, vel = orbiting(0.0, 6600.0 * (1.0 + 49.0 * np.arange(72) / 71.0))
    return Scenario("E", table, [MU0, MU1, MU2], 0.0, pos, vel, dict(h_init=5.0, h_max=400.0, tol_pos=1e-5, tol_vel=1e-5),
                    [("propagate", 5000.0)], _live_e, py_craft=[0, 7, 31, 63, 64, 71])


# ---- F ----------------------------------------------------------------------------------------------------------------------------
F_BURNS = [(4096.0, 4096.0 + 128.0, [3e-4, -1e-4, 2e-4], 0), (4096.0 + 320.0, 4096.0 + 448.0, [-2e-4, 1e-4, 1e-4], 0)]


def _live_f(sc, method, res):
    assert sc.table[0][0] == F_BURNS[0][0] and sc.table[1][0] == 64.0          # tau == 0 at the first burn's start
    for i, r in enumerate(res):
        assert r["status"] == 0, (sc.name, method, i, r["status"])
        kt = r["craft"].knots()[0]
        for b in F_BURNS:
            assert b[0] in kt and b[1] in kt and (b[1] - 4096.0) % 64.0 == 0.0, (sc.name, method, i)


def scenario_f():
    table = _table_abc(n0=20, n1=10, n2=6)
    pos, vel = orbiting(0.0, [7000.0, 9000.0, 26000.0])
    return Scenario("F", table, [MU0, MU1, MU2], 4096.0, pos, vel, dict(h_init=40.0, h_max=64.0, tol_pos=1e3, tol_vel=1e3),
                    [("propagate", 4096.0 + 700.0)], _live_f, burns=[list(F_BURNS) for _ in range(3)])


def scenarios():
    return [scenario_a(), scenario_b_dyadic(), scenario_b_inexact(), scenario_c()] + scenarios_d() + [scenario_e(), scenario_f()]


def planted_epochs(sc, b):
    """where the direct evaluators are compared on body b: start, every boundary and its two neighbours, start + span and its upper
    neighbour, +-inf (at most 40 boundaries of a long table, the last ones included)"""
    s, iv, n = sc.table[0][b], sc.table[1][b], len(sc.table[2][b])
    ks = sorted(set(list(range(0, min(n, 20) + 1)) + list(range(max(n - 20, 0), n + 1))))
    out = []
    for k in ks:
        t = s + iv * float(k)
        out += [np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)]
    return np.array(out + [-np.inf, np.inf])
