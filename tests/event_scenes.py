"""Scenes for the event search -- the app's SpacecraftSolout: sphere-of-influence transitions and apsides per accepted step -- with the cold
arms PLANTED: shared by tests/test_event_scenes.py (CPU: the C oracle against the Python restatement) and tests/test_gpu_craft_events.py
(device against the C oracle). A plain module, no fixtures; the table helpers' idiom is tests/synthetic_tables.py's.

Why: k_craft_events (csrc/craft_events.hip, with soi_at_except and tr_insert of csrc/craft_events.h) is compared elsewhere only on the
Mars transfer, whose three transitions never nest, never share a step, never overwrite, never land in front of one another and always
have a root sphere to fall back to. These scenes are built the other way round: every body but (in T and F-ap) body 0 has mu == 0, so the
craft's knots do not depend on where the bodies are, and the spheres are placed on a trajectory that is known beforehand. A body at rest
is one polynomial of TWO rows [p, 0] (a single row evaluates to c0 * tau + c0 in Polynomial::eval_and_deriv).

The craft of the line scenes fly along +x from (2048, 3, 0) at 1 km/s with h_init == h_max, so a knot lies every h_max km (plus ~1e-12:
the stage weights do not sum to 1 in binary64 -- whatever must hit a knot EXACTLY is planted from the oracle's own knots, in two passes).

Scene -> the arm it is there for
  N   nested spheres: root (r = inf) > body 1 (r = 1024) > bodies 3 and 2 (r = 64, 128), in 64 s steps: Descending into an inner sphere,
      the Ascending arm's soi_at_except landing in the parent and, at the end, in the root; apsides about an inner body while inside it.
      N-512: the same in 512 s steps: the inner spheres are stepped over (same sign at both ends of the step): [0, 1, 0].
  O   one step, several bodies: three overlapping spheres (bodies 1, 2, 3) entered inside ONE 512 s step, in time order 3, 2, 1: every
      insertion after the first lands in FRONT of entries of the same step (the shift loop of tr_insert); their exits find one another
      (Ascending into a sphere that is not the parent, and the same-body rule). Twin bodies 4 and 5 (one sphere) are entered in one step
      and left in the next: the twin of the higher index overwrites the other at the equal time (the Ok(i) arm), in body order.
  D   dedupe: the craft starts inside overlapping spheres A (body 2, 8 km away) and B (body 1, 140 km away); leaving B finds A again
      and nothing is inserted (`*c == entity`): [A, root].
  R   no root: every radius finite; the craft starts in no sphere (ntr == 0: the apsis loop does not run), enters body 1 later
      (starting_at's lo == 0, ta = t in the first window) and leaves it for nothing (the list stays at one entry, whose window goes on).
  Z   zeros (Verner87, planted from that method's knots): craft 0 leaves a sphere exactly on a knot (f(t1) == +0, next step f(t0) == +0),
      craft 1 enters one exactly on a knot (f(t0) == +0, the interior negative), craft 2 starts exactly on a sphere (d2 == r * r in
      find_soi at knot 0: outside), craft 3 (flying along +x) and craft 4 (along -x) have a body exactly abeam at a knot, at
      (0, 300, 400) from it: the radial velocity there is (+0 * 1) + (-300 * +0) + (-400 * +0) == +0 for craft 3 and -0.0 for craft 4,
      whose periapsis is found at t0 of the step after the knot with signum(-0.0) == -1 (`f0 < 0.0` would call it an apoapsis). 3-4-5
      offsets make the squares exact. (A craft exactly AT a body's centre on a knot cannot be continued: the next stage divides 0 by 0
      even for mu == 0 and the sweep stops, so the bodies are abeam.)
  W   more than 64 bodies: 65 and 130, the crossed ones (3 and 64; 3, 64, 70 and 129) in every tile of the wave form and out of order along
      the line, entered in one step and left in the next; the rest are far bodies with tiny spheres.
  T   thread lanes: 136 craft (two full waves and a part) on eccentric orbits about a massive body 0 at rest, semi-major axes spread over
      a factor of 40 and stored in scrambled order; body 0's sphere is finite, so some craft cross it, some stay inside and some never
      meet a sphere; massless bodies at rest with small nested spheres sit on some of the orbits. Neighbouring lanes have different
      event histories, and in the dealt thread form (batches of >= 128 craft) slot_of is a real permutation: knots are read from column
      slot_of[i], event slabs from column i. The permutation cannot be read from outside; a wrong column shows as wrong events.
  F-tr  full inside a step: scene O with max_transitions = 3: the step with three entries starts with one entry in the slab, so the third
      insertion is refused from INSIDE the step, which is searched again after the drain. F-ap: the apsis side (max_apsides = 3) on a
      short-period orbit with a small h_max.

Unreachable from a sweep, and left out: event_f returning false at a knot (the sweep fails with EvalFailed first), the dt == 0 arm of
CubicHermite::new (an accepted step has t + h != t), NaN epochs."""
import math

import numpy as np

import synthetic_tables as syn

MU_EARTH = 398600.4418
INF = float("inf")
METHODS = syn.METHODS
SPAN = 2.0 ** 20                                   # every body: one polynomial from t = 0 to 2^20 s
EVENTS_FULL = 7


def rest_table(points):
    """bodies at rest at `points`: (start, interval, polys) with one polynomial of two rows [p, 0] each"""
    return ([0.0] * len(points), [SPAN] * len(points), [[np.array([np.asarray(p, dtype=np.float64), np.zeros(3)])] for p in points])


class Scene(syn.Scenario):
    """a syn.Scenario plus the sphere radii and the event slab sizes; liveness(scene, method, results) asserts on the ORACLE's lists"""

    def __init__(self, name, points, mu, soi, pos, vel, params, calls, liveness, max_tr=16, max_ap=64, drain=False, **kw):
        super().__init__(name, rest_table(points), mu, 0.0, pos, vel, params, calls, liveness, **kw)
        self.points = np.asarray(points, dtype=np.float64)
        self.soi = np.asarray(soi, dtype=np.float64)
        self.max_tr, self.max_ap, self.drain = max_tr, max_ap, drain
        assert len(self.soi) == self.n_bodies == len(self.points)


def run_oracle(sc, method, solution):
    """the scene on orc.Craft with the SpacecraftSolout -> per craft dict(status, craft)"""
    from oracle import orc
    p = sc.params
    out = []
    for i in range(sc.n):
        c = orc.Craft(solution, sc.mu, sc.t0[i], sc.pos[i], sc.vel[i], method, h_init=p["h_init"], h_max=p["h_max"], tol_pos=p["tol_pos"],
                      tol_vel=p["tol_vel"], soi_radius=sc.soi)
        out.append(dict(status=syn._run_calls(sc, c.step_to, c.step), craft=c))
    return out


def run_python(sc, method, i, table=None):
    """craft i of the scene on pyoracle.Craft -> (status, craft)"""
    from oracle import pyoracle as po
    p = sc.params
    c = po.Craft(table if table is not None else syn.python_table(sc.table), sc.mu, float(sc.t0[i]), sc.pos[i], sc.vel[i], method,
                 p["tol_pos"], [], h_init=p["h_init"], soi=[float(r) for r in sc.soi])
    c.h_max, c.tol_pos, c.tol_vel = p["h_max"], p["tol_pos"], p["tol_vel"]

    def step_to(t):
        while not c.knots[-1][0] >= t:
            st = c.step()
            if st:
                return st
        return 0
    return syn._run_calls(sc, step_to, c.step), c


def bodies_of(r):
    return [int(b) for b in r["craft"].transitions()[1]]


def per_step(r):
    """how many of the craft's transitions lie in each step [knot k, knot k + 1)"""
    kt = r["craft"].knots()[0]
    tt = r["craft"].transitions()[0]
    return np.bincount(np.clip(np.searchsorted(kt, tt, side="right") - 1, 0, len(kt) - 1), minlength=len(kt))


def _all_ok(sc, method, res):
    for i, r in enumerate(res):
        assert r["status"] == 0, (sc.name, method, i, r["status"])


LINE_POS, LINE_VEL = [[2048.0, 3.0, 0.0]], [[1.0, 0.0, 0.0]]


def _line(h):
    return dict(h_init=h, h_max=h, tol_pos=1e3, tol_vel=1e3)


# ---- N ----------------------------------------------------------------------------------------------------------------------------
N_POINTS = [[0.0, 0.0, 0.0], [4096.0, 0.0, 0.0], [4352.0, 0.0, 0.0], [3840.0, 0.0, 0.0]]
N_SOI = [INF, 1024.0, 128.0, 64.0]


def _live_n(want, peri):
    def live(sc, method, res):
        _all_ok(sc, method, res)
        assert bodies_of(res[0]) == want, (sc.name, method, bodies_of(res[0]))
        at, ad, ab, ak = res[0]["craft"].apsides()
        assert sorted(set(ab.tolist())) == peri and (ak == 0).all(), (sc.name, method, ab, ak)      # periapsides about the inner bodies
    return live


def scenes_n():
    return [Scene("N", N_POINTS, [0.0] * 4, N_SOI, LINE_POS, LINE_VEL, _line(64.0), [("propagate", 8192.0)],
                  _live_n([0, 1, 3, 1, 2, 1, 0], [1, 2, 3]), max_knots=160),
            Scene("N-512", N_POINTS, [0.0] * 4, N_SOI, LINE_POS, LINE_VEL, _line(512.0), [("propagate", 8192.0)], _live_n([0, 1, 0], [1]),
                  max_knots=32)]


# ---- O ----------------------------------------------------------------------------------------------------------------------------
def sphere(entry, exit_):
    """(centre, radius) of a sphere on the x axis that the line y = 3 enters near x = entry and leaves near x = exit_"""
    return [(entry + exit_) / 2.0, 0.0, 0.0], (exit_ - entry) / 2.0


def _table_o():
    """knots at x = 2048 + 512 k. Bodies 1, 2, 3 are entered in step 3 (3584 .. 4096) at x = 4050, 4000, 3950 and left in step 4 at
    4250, 4440, 4570; the twins 4 and 5 are entered in step 1 at 3000 and left in step 2 at 3200"""
    pts, soi = [[0.0, 0.0, 0.0]], [INF]
    for entry, exit_ in ((4050.0, 4250.0), (4000.0, 4440.0), (3950.0, 4570.0), (3000.0, 3200.0), (3000.0, 3200.0)):
        c, r = sphere(entry, exit_)
        pts.append(c), soi.append(r)
    return pts, soi


def _live_o(sc, method, res):
    _all_ok(sc, method, res)
    r = res[0]
    tt, tb = r["craft"].transitions()
    steps = per_step(r)
    assert steps.max() >= 3, (sc.name, method, steps)
    k = int(np.argmax(steps >= 3))
    kt = r["craft"].knots()[0]
    inside = tb[(tt >= kt[k]) & (tt < kt[k + 1])]
    assert list(inside[:3]) == [3, 2, 1], (sc.name, method, inside)                 # time order against body order
    # the twins: one entry at their common entry time, and it names the later twin; their exit lies in the next step
    assert np.count_nonzero(tb == 5) == 1 and list(tb[:3]) == [0, 5, 4], (sc.name, method, tb)
    t5, t4 = tt[1], tt[2]
    assert np.searchsorted(kt, t5, side="right") + 1 == np.searchsorted(kt, t4, side="right"), (sc.name, method, t5, t4)
    assert list(tb) == [0, 5, 4, 3, 2, 1, 3, 0], (sc.name, method, tb)


def scene_o(name="O", **kw):
    pts, soi = _table_o()
    return Scene(name, pts, [0.0] * 6, soi, LINE_POS, LINE_VEL, _line(512.0), [("propagate", 6144.0)], _live_o, max_knots=32, **kw)


# ---- D ----------------------------------------------------------------------------------------------------------------------------
def _live_d(sc, method, res):
    _all_ok(sc, method, res)
    assert bodies_of(res[0]) == [2, 0], (sc.name, method, bodies_of(res[0]))          # no second entry for A when B is left
    kt = res[0]["craft"].knots()[0]
    assert len(kt) > 12


def scene_d():
    pts = [[0.0, 0.0, 0.0], [2048.0 + 140.0, 3.0, 0.0], [2048.0 + 8.0, 3.0, 0.0]]          # root, B, A
    return Scene("D", pts, [0.0] * 3, [INF, 200.0, 500.0], LINE_POS, LINE_VEL, _line(64.0), [("propagate", 1024.0)], _live_d, max_knots=32)


# ---- R ----------------------------------------------------------------------------------------------------------------------------
def _live_r(sc, method, res):
    _all_ok(sc, method, res)
    tt, tb = res[0]["craft"].transitions()
    assert not np.isinf(sc.soi).any()
    assert list(tb) == [1] and tt[0] > 4 * 64.0, (sc.name, method, tt, tb)             # several steps in no sphere, one entry ever after
    at, ad, ab, ak = res[0]["craft"].apsides()
    assert list(ab) == [1] and list(ak) == [0]
    kt = res[0]["craft"].knots()[0]
    assert kt[-1] > tt[0] + 400.0 + 4 * 64.0                                           # and several steps after the exit


def scene_r():
    pts = [[-5000.0, 0.0, 0.0], [3000.0, 0.0, 0.0], [9000.0, 500.0, 0.0]]
    return Scene("R", pts, [0.0] * 3, [100.0, 200.0, 50.0], LINE_POS, LINE_VEL, _line(64.0), [("propagate", 2048.0)], _live_r, max_knots=48)


# ---- Z ----------------------------------------------------------------------------------------------------------------------------
Z_KNOT = 20
Z_START = np.array([[2048.0, 3.0, 0.0], [2048.0, 100003.0, 0.0], [2048.0, 200003.0, 0.0], [2048.0, 300003.0, 0.0], [8192.0, 400003.0, 0.0]])
Z_VEL = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
Z_ABEAM = np.array([0.0, 300.0, 400.0])
Z_BODY = {"exit": 1, "entry": 2, "start": 3, "plus": 4, "minus": 5}


def _z_knots():
    """pass one: the craft's knots on Verner87 (the bodies are massless: any table gives these knots)"""
    from oracle import orc
    sol = orc.Solution.from_parts(*rest_table([[0.0, 0.0, 0.0]]))
    out = []
    for p, v in zip(Z_START, Z_VEL):
        c = orc.Craft(sol, [0.0], 0.0, p, v, "Verner87", h_init=64.0, h_max=64.0, tol_pos=1e3, tol_vel=1e3)
        assert c.step_to(64.0 * 40) == 0
        out.append(c.knots())
    return out


def _d2_minus_r2(p, b, r):
    """soi_distance_squared_at in numpy's binary64, the reference's order of operations"""
    d = np.asarray(p, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - r * r


def _live_z(sc, method, res):
    _all_ok(sc, method, res)
    k = Z_KNOT
    knots = [r["craft"].knots() for r in res]
    for i in range(sc.n):
        assert knots[i][0][k] == 64.0 * k
    # craft 0: on body 1's sphere at knot k, going out: found inside the step before, Ascending (the root follows)
    z = _d2_minus_r2(knots[0][1][k], sc.points[1], sc.soi[1])
    assert z == 0.0 and not np.signbit(z) and _d2_minus_r2(knots[0][1][k - 1], sc.points[1], sc.soi[1]) < 0.0
    tt, tb = res[0]["craft"].transitions()
    assert list(tb) == [0, 1, 0] and 64.0 * (k - 1) < tt[2] < 64.0 * k and 64.0 * k - tt[2] < 1e-3, (tt, tb)
    # craft 1: on body 2's sphere at knot k, going in: found in the step after it, at its t0
    z = _d2_minus_r2(knots[1][1][k], sc.points[2], sc.soi[2])
    assert z == 0.0 and not np.signbit(z) and _d2_minus_r2(knots[1][1][k + 1], sc.points[2], sc.soi[2]) < 0.0
    assert _d2_minus_r2(knots[1][1][k - 1], sc.points[2], sc.soi[2]) > 0.0
    tt, tb = res[1]["craft"].transitions()
    assert list(tb[:2]) == [0, 2] and tt[1] == 64.0 * k, (tt, tb)
    # craft 2: on body 3's sphere at knot 0, going out: `<` keeps it outside, in the root, and f(t0) == +0 of the first step is no crossing
    z = _d2_minus_r2(knots[2][1][0], sc.points[3], sc.soi[3])
    assert z == 0.0 and not np.signbit(z)
    tt, tb = res[2]["craft"].transitions()
    assert list(tb) == [0] and tt[0] == 0.0, (tt, tb)
    # craft 3 / craft 4: a body abeam at knot k; the radial velocity there is +0 / -0.0. Craft 4's periapsis is found from the knot as t0
    # with ascending == True (kind 0)
    for i, body, zero_is_negative in ((3, 4, False), (4, 5, True)):
        rp = knots[i][1][k] - sc.points[body]
        assert list(rp) == [0.0, -300.0, -400.0] and not np.signbit(rp[0]), (i, rp)
        rv = knots[i][2][k] - np.zeros(3)
        f = (rp[0] * rv[0] + rp[1] * rv[1]) + rp[2] * rv[2]
        assert f == 0.0 and bool(np.signbit(f)) == zero_is_negative, (i, f, rv)
        at, ad, ab, ak = res[i]["craft"].apsides()
        mine = np.flatnonzero(ab == body)
        assert len(mine) >= 1 and (ak[mine] == 0).all(), (i, at, ab, ak)
        if zero_is_negative:
            assert at[mine[-1]] == 64.0 * k, (i, at)


def scene_z():
    k = Z_KNOT
    knots = _z_knots()
    off = np.array([300.0, 400.0, 0.0])
    pts = [[0.0, 0.0, 0.0],
           knots[0][1][k] - off,                   # behind the craft: it leaves at knot k
           knots[1][1][k] + off,                   # ahead of the craft: it enters at knot k
           Z_START[2] - off,                       # behind the craft at knot 0
           knots[3][1][k] + Z_ABEAM, knots[4][1][k] + Z_ABEAM]
    return Scene("Z", pts, [0.0] * 6, [INF, 500.0, 500.0, 500.0, 700.0, 700.0], Z_START, Z_VEL, _line(64.0), [("propagate", 64.0 * 40)],
                 _live_z, max_knots=64, methods=("Verner87",))


# ---- W ----------------------------------------------------------------------------------------------------------------------------
def _live_w(planted):
    def live(sc, method, res):
        _all_ok(sc, method, res)
        tb = bodies_of(res[0])
        assert set(planted) <= set(tb), (sc.name, method, tb)
        steps = per_step(res[0])
        assert np.count_nonzero(steps) <= 3 and len(tb) >= len(planted) + 2, (sc.name, method, steps, tb)      # knot 0 + at most two steps
    return live


def scene_w(nb, planted):
    """the planted bodies are entered in step 3 (3584 .. 4096), in an order along the line that is not the body order, and left in step 4"""
    pts, soi = [[0.0, 0.0, 0.0]], [INF]
    for j in range(1, nb):
        a = 0.7 * j
        pts.append([1.0e6 * math.cos(a), 1.0e6 * math.sin(a), 3.0e5 + j]), soi.append(1.0 + 0.01 * j)
    entries = {3: (4050.0, 4300.0), 64: (3900.0, 4500.0), 70: (3950.0, 4200.0), 129: (4000.0, 4400.0)}
    for b in planted:
        pts[b], soi[b] = sphere(*entries[b])
    return Scene(f"W-{nb}", pts, [0.0] * nb, soi, LINE_POS, LINE_VEL, _line(512.0), [("propagate", 6144.0)], _live_w(planted), max_knots=32)


# ---- T ----------------------------------------------------------------------------------------------------------------------------
T_N, T_END, T_SOI0 = 136, 30000.0, 60000.0
T_PLANTED = range(0, T_N, 9)                       # the craft whose orbits get a pair of nested spheres


def _t_craft():
    """eccentric orbits about the origin: a = 7000 .. 280 000 km in scrambled order, started at periapsis in different planes"""
    rng = np.random.default_rng(20261019)
    a = 7000.0 * 40.0 ** (rng.permutation(T_N) / (T_N - 1.0))
    e = 0.15 + 0.6 * rng.random(T_N)
    pos, vel = [], []
    for i in range(T_N):
        ang = 0.61 * i
        u = np.array([math.cos(ang), math.sin(ang), 0.2 * math.sin(1.3 * i)])
        u /= np.linalg.norm(u)
        w = np.cross([0.0, 0.0, 1.0], u)
        w /= np.linalg.norm(w)
        rp = a[i] * (1.0 - e[i])
        pos.append(rp * u), vel.append(math.sqrt(MU_EARTH * (1.0 + e[i]) / rp) * w)
    return a, np.array(pos), np.array(vel)


T_PARAMS = dict(h_init=30.0, h_max=INF, tol_pos=1e-2, tol_vel=1e-5)


def _t_points(method, pos, vel):
    """pass one: the orbits without the small bodies (massless: they do not move the knots); a pair of concentric spheres on a knot in
    the middle of every planted craft's run, offset from the knot so that the craft passes the centre at a distance"""
    from oracle import orc
    sol = orc.Solution.from_parts(*rest_table([[0.0, 0.0, 0.0]]))
    pts, soi = [[0.0, 0.0, 0.0]], [T_SOI0]
    for i in T_PLANTED:
        c = orc.Craft(sol, [MU_EARTH], 0.0, pos[i], vel[i], method, **T_PARAMS)
        assert c.step_to(T_END) == 0
        kt, kp, kv = c.knots()
        k = len(kt) // 2
        r = 0.8 * float(np.linalg.norm(kp[k + 1] - kp[k]))
        centre = kp[k] + r * np.array([0.1, 0.14, 0.2])
        pts += [centre, centre]
        soi += [r, 0.5 * r]
    return pts, soi


def _live_t(sc, method, res):
    _all_ok(sc, method, res)
    pairs, about, none = set(), set(), 0
    for r in res:
        tt, tb = r["craft"].transitions()
        at, ad, ab, ak = r["craft"].apsides()
        pairs.add((len(tt), len(at)))
        about |= set(ab.tolist())
        none += len(tt) == 0 and len(at) == 0
        assert len(r["craft"].knots()[0]) <= sc.max_knots and len(tt) <= sc.max_tr - 2 and len(at) <= sc.max_ap - 2
    assert len(pairs) >= 20 and none >= 3 and len(about) >= 2 and 0 in about, (sc.name, method, len(pairs), none, about)
    assert sc.n >= 136 and sc.a.max() / sc.a.min() >= 30.0


def scene_t(method):
    a, pos, vel = _t_craft()
    pts, soi = _t_points(method, pos, vel)
    sc = Scene(f"T-{method}", pts, [MU_EARTH] + [0.0] * (len(pts) - 1), soi, pos, vel, T_PARAMS, [("propagate", T_END)], _live_t,
               max_tr=40, max_ap=24, max_knots=400, methods=(method,), py_craft=[0, 9, 63, 64, 135])
    sc.a = a
    return sc


# ---- F ----------------------------------------------------------------------------------------------------------------------------
def _live_f_ap(sc, method, res):
    _all_ok(sc, method, res)
    at, ad, ab, ak = res[0]["craft"].apsides()
    assert len(at) >= 6 and set(ak.tolist()) == {0, 1}, (sc.name, method, at, ak)


def scene_f_ap():
    rp, e = 7000.0, 0.1
    period = 2.0 * math.pi * math.sqrt((rp / (1.0 - e)) ** 3 / MU_EARTH)
    return Scene("F-ap", [[0.0, 0.0, 0.0]], [MU_EARTH], [INF], [[rp, 0.0, 0.0], [0.0, 1.1 * rp, 0.0]],
                 [[0.0, math.sqrt(MU_EARTH * (1.0 + e) / rp), 0.0], [-math.sqrt(MU_EARTH * (1.0 + e) / (1.1 * rp)), 0.0, 0.0]],
                 dict(h_init=30.0, h_max=200.0, tol_pos=1e-3, tol_vel=1e-6), [("propagate", 3.3 * period)], _live_f_ap, max_tr=3, max_ap=3,
                 drain=True, max_knots=256)


def scenes():
    """the scenes that run in one go (events compared list against list)"""
    return scenes_n() + [scene_o(), scene_d(), scene_r(), scene_z(), scene_w(65, [3, 64]), scene_w(130, [3, 64, 70, 129])] + \
        [scene_t(m) for m in METHODS]


def drain_scenes():
    """the scenes whose slabs are too small on purpose: read, reset_events, propagate again, and merge"""
    return [scene_o("F-tr", max_tr=3, max_ap=8, drain=True), scene_f_ap()]


def merge_transitions(reads):
    """the lists read from a drained batch, oldest first, merged the way a caller holding the reference's types would: every entry
    through SoiTransitions::insert. reads: lists of (time, body)"""
    from oracle import pyoracle as po
    out = []
    for read in reads:
        for time, body in read:
            po.transitions_insert(out, float(time), int(body))
    return out


def merge_apsides(reads):
    """Apsides::insert for every entry: by time, an equal time overwrites. reads: lists of (time, distance, body, kind)"""
    import bisect
    out = []
    for read in reads:
        for rec in read:
            at = [a[0] for a in out]
            j = bisect.bisect_left(at, rec[0])
            if j < len(at) and at[j] == rec[0]:
                out[j] = tuple(rec)
            else:
                out.insert(j, tuple(rec))
    return out
