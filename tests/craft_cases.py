"""What the device tests share: bit-pattern comparison, the Mars-transfer ship and its perturbed copies, a system propagated on the
device and in the oracle, the knots of a whole batch as host arrays, the restatement of one plot, and the two snapshots of a batch.
A plain module (like hooks.py): test modules import what they use; an imported fixture keeps its module scope, so every module
builds its own device objects."""
import numpy as np
import pytest

from conftest import SYSTEMS, load_system
from ephemeris_explorer_amd.systems import parse_epoch
from oracle import orc
from oracle import pyoracle as po

SHIP = SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json"
DAY = 86400.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def perturbed(ship, n, seed):
    """craft 0 is the ship itself; the others differ by normal(0, 1 km / 1e-4 km/s) per component"""
    rng = np.random.default_rng(seed)
    pos = ship.pos + rng.normal(0.0, 1.0, size=(n, 3))
    vel = ship.vel + rng.normal(0.0, 1e-4, size=(n, 3))
    pos[0], vel[0] = ship.pos, ship.vel
    return pos, vel


def propagated(gpu, name, end):
    """system `name` to `end` on the device and in the oracle, the two solutions of the same extent (bit-identical:
    test_gpu_parity.py) -> (system, device Solution, device Ephemeris, oracle solution)"""
    s = load_system(name)
    sol = gpu.NBodyPropagator.from_system(s).propagate(end)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    assert o.step_to(end) == 0
    osol = o.take_solution()
    for b in range(s.n):
        assert sol.info(b) == osol.info(b)
    return s, sol, gpu.Ephemeris(sol, s.mu), osol


@pytest.fixture(scope="module")
def simple_system(gpu):
    """10-body 1950 system, QuinlanTremaine12 6 h, two years of ephemeris: on the GPU and in the oracle, like
    ephemeris/tests/spacecraft_propagation.rs:401-409."""
    return propagated(gpu, "simple_solar_system_2433282.5", parse_epoch("1952-01-01 00:00:00"))


def gathered_knots(batch, nknots):
    """every craft's knots as eph_plot_points wants them -- concatenated [knot] / [knot][3] arrays with (first, count) per craft --
    from one bulk read of the slab's first rows plus one eph_craft_batch_knots call for each of the few long craft"""
    rows = min(int(nknots.max()), 512)
    t, y = batch.knot_slabs(0, rows)
    live = (np.arange(rows)[None, :] < nknots[:, None])                                 # [craft][k]
    first = np.concatenate([[0], np.cumsum(nknots)[:-1]]).astype(np.int64)
    kt, kp, kv = np.zeros(int(nknots.sum())), np.zeros((int(nknots.sum()), 3)), np.zeros((int(nknots.sum()), 3))
    short = nknots <= rows
    dest = (first[:, None] + np.arange(rows)[None, :])[live & short[:, None]]
    yt = y.transpose(2, 0, 1)                                                           # [craft][k][6]
    kt[dest] = t.T[live & short[:, None]]
    kp[dest] = yt[live & short[:, None]][:, :3]
    kv[dest] = yt[live & short[:, None]][:, 3:]
    for c in np.flatnonzero(~short):
        ct, cp, cv = batch.knots(int(c), nknots[c])
        kt[first[c]:first[c] + nknots[c]], kp[first[c]:first[c] + nknots[c]], kv[first[c]:first[c] + nknots[c]] = ct, cp, cv
    return (kt, kp, kv), first, nknots.astype(np.int64)


def oracle_plot(s, osol, knots, view, rq):
    """compute_plot_points_parallel :318-374 for one plot, evaluations by the oracle."""
    def bounds(body):
        st, iv, n = osol.info(body)
        return st, st + iv * float(n), n
    if rq.get("source_body", -1) >= 0:
        tb = bounds(rq["source_body"])
    else:
        first, count = rq["knots"]
        kt = knots[0][first:first + count]
        tb = (kt[0], kt[-1], len(kt) - 1) if len(kt) else (po.EPOCH_MIN, po.EPOCH_MAX, 0)
    ref = rq.get("reference_body", -1)
    rb = bounds(ref) if ref >= 0 else None
    if not rq.get("enabled", 1):
        return "ok", []
    win = po.plot_window(tb, rb, rq["start"], rq["end"], rq.get("bound", 0), view["current"])
    if win is None:
        return "ok", []
    tr = po.Vec(0.0, 0.0, 0.0)
    if ref >= 0:
        tc = min(max(view["current"], rb[0]), rb[1])
        tr = po.Vec(*osol.eval(ref, tc, with_velocity=False))
    m = np.asarray(view.get("grid_matrix3", np.eye(3)), dtype=np.float64)
    ax = [po.Vec(*m[:, c]) for c in range(3)]
    gt, cell = po.Vec(*view.get("grid_translation", (0.0,) * 3)), po.Vec(*view.get("cell_offset", (0.0,) * 3))
    mul = lambda v: (ax[0] * v[0] + ax[1] * v[1]) + ax[2] * v[2]      # noqa: E731  glam DMat3::mul_vec3

    def evaluate(t):
        rp, rv = po.Vec(0.0, 0.0, 0.0), po.Vec(0.0, 0.0, 0.0)
        if ref >= 0:
            r = osol.eval(ref, t)
            if r is None:
                return None
            rp, rv = po.Vec(*r[0]), po.Vec(*r[1])
        if rq.get("source_body", -1) >= 0:
            r = osol.eval(rq["source_body"], t)
        else:
            first, count = rq["knots"]
            r = orc.hermite_eval(knots[0][first:first + count], knots[1][first:first + count], knots[2][first:first + count], t)
        if r is None:
            return None
        pos = (po.Vec(*r[0]) - rp) + tr
        vel = (po.Vec(*r[1]) - rv) + po.Vec(0.0, 0.0, 0.0)
        return mul(pos - cell) + gt, mul(vel)
    return po.plot_points_new(evaluate, win[0], win[1], po.Vec(*view["camera_position"]), rq["tan2_angular_resolution"],
                              rq["max_points"])


# The two snapshots stay apart: a reader must leave the slabs as they are (read in bulk, events always on in those tests), a restart
# may rewrite any craft's knots (read per craft, as check_craft does) and runs with and without events.
def snapshot_of_slabs(batch):
    """everything a reader must leave alone: the summary records, the live part of the knot slabs, the event counts and lists"""
    rec = batch.summary()
    t, y = batch.knot_slabs()
    live = np.arange(t.shape[0])[:, None] < rec["nknots"][None, :]
    counts = batch.event_counts()
    ev = [batch.events(c, counts) for c in range(batch.n)]
    return (rec.tobytes(), t[live].tobytes(), y[np.broadcast_to(live[:, None, :], y.shape)].tobytes(), [np.asarray(x).tobytes() for x in counts],
            [np.asarray(a).tobytes() for e in ev for part in e for a in part])


def snapshot_of_knots(batch):
    """everything a restart may change: the summary records, every craft's knots and (if enabled) event lists"""
    rec = batch.summary().tobytes()
    nk = batch.status()["nknots"]
    kn = [tuple(bits(x).tobytes() for x in batch.knots(c, nk[c])) for c in range(batch.n)]
    try:
        counts = batch.event_counts()
    except Exception:
        return rec, kn, None
    ev = [tuple(np.asarray(x).tobytes() for part in batch.events(c, counts) for x in part) for c in range(batch.n)]
    return rec, kn, (tuple(x.tobytes() for x in counts), ev)
