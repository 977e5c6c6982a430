"""-m gpu: the adaptive plot sampler -- eph_plot_points against the Python restatement of
compute_plot_points_parallel / PlotPoints::new / angular_distance (ephemeris_explorer/src/ui/world/plot.rs:93-149,272-374,
429-436), whose trajectory evaluations come from the C oracle. Epochs bit-identical, positions identical f32."""
import numpy as np
import pytest

from conftest import SYSTEMS, load_system
from craft_cases import oracle_plot
from ephemeris_explorer_amd.systems import load_ship, parse_epoch
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(gpu):
    s = load_system("simple_solar_system_2433282.5")
    end = parse_epoch("1950-09-01 00:00:00")
    g = gpu.NBodyPropagator.from_system(s)
    sol = g.propagate(end)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    assert o.step_to(end) == 0
    osol = o.take_solution()
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    c = orc.Craft(osol, s.mu, ship.start, ship.pos, ship.vel, "Verner87")
    assert c.step_to(ship.start + 20 * 86400.0) == 0
    return s, gpu.Ephemeris(sol, s.mu), osol, c.knots()


def test_plot_points_match_the_restatement(gpu, scene):
    s, eph, osol, knots = scene
    nk = len(knots[0])
    sun, earth, moon, mars = (s.names.index(x) for x in ("Sun", "Earth", "Moon", "Mars"))
    t0 = s.epoch
    day = 86400.0
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])            # a rotation (exact-ish entries)
    views = [
        {"camera_position": (1.2e8, -3.0e8, 2.0e8), "current": t0 + 30 * day},
        {"camera_position": (5.0e5, 2.0e5, -3.0e5), "current": t0 + 3 * day, "grid_matrix3": rot,
         "grid_translation": (10.0, -20.0, 5.0), "cell_offset": (1.0e6, 2.0e6, -5.0e5)},
    ]
    res = float(np.float32(1.0) * np.float32(0.000290888) * np.float32(0.7853982))          # threshold * ARC_MINUTE * fov
    requests = [
        {"source_body": earth, "reference_body": -1, "start": t0, "end": t0 + 200 * day, "tan2_angular_resolution": res, "max_points": 4000},
        {"source_body": moon, "reference_body": earth, "start": t0 - day, "end": t0 + 90 * day, "tan2_angular_resolution": res, "max_points": 4000},
        {"source_body": mars, "reference_body": sun, "start": t0, "end": t0 + 1e9, "bound": 1, "tan2_angular_resolution": res * 4, "max_points": 4000},
        {"source_body": earth, "reference_body": sun, "start": t0, "end": t0 + 100 * day, "bound": 2, "tan2_angular_resolution": res, "max_points": 4000},
        {"knots": (0, nk), "reference_body": earth, "start": t0, "end": t0 + 30 * day, "tan2_angular_resolution": res, "max_points": 4000},
        {"knots": (0, nk), "reference_body": -1, "start": t0, "end": t0 + 30 * day, "tan2_angular_resolution": res * 0.25, "max_points": 64},   # max_points cuts it
        {"knots": (5, 40), "reference_body": moon, "start": t0, "end": t0 + 30 * day, "tan2_angular_resolution": res, "max_points": 4000},
        {"source_body": moon, "reference_body": earth, "start": t0, "end": t0 + 10 * day, "enabled": 0, "tan2_angular_resolution": res, "max_points": 100},
        {"source_body": moon, "reference_body": -1, "start": t0 + 50 * day, "end": t0 + 40 * day, "tan2_angular_resolution": res, "max_points": 100},  # min >= max
        {"knots": (0, 1), "reference_body": -1, "start": t0, "end": t0 + day, "tan2_angular_resolution": res, "max_points": 100},                   # one knot: no segment
        {"source_body": sun, "reference_body": -1, "start": t0, "end": t0 + 60 * day, "tan2_angular_resolution": res, "max_points": 0},
    ]
    total = 0
    for view in views:
        got = gpu.plot_points(eph, view, requests, knots)
        for i, (rq, (st, failed_at, t, xyz)) in enumerate(zip(requests, got)):
            kind, want = oracle_plot(s, osol, knots, view, rq)
            assert kind == "ok" and st == 0, (i, kind, st)
            assert len(t) == len(want), (i, len(t), len(want))
            wt = np.array([w[0] for w in want])
            wx = np.array([w[1] for w in want], dtype=np.float32).reshape(-1, 3)
            assert np.array_equal(t.view(np.uint64), wt.view(np.uint64)), i
            assert np.array_equal(xyz.view(np.uint32), wx.view(np.uint32)), i
            total += len(t)
    assert total > 300
    # the adaptive sampler does what it is for: the step follows the curvature seen from the camera, not a fixed rate
    assert len(got[1][2]) > 20 and np.ptp(np.diff(got[1][2])) > 0.1 * np.diff(got[1][2]).mean()


def test_plot_points_argument_errors(gpu, scene):
    """max_points beyond the capacity the caller provided, bodies out of range: refused before anything runs."""
    import ctypes as C
    s, eph, osol, knots = scene
    L = gpu._lib()
    v = gpu.PlotView()
    v.camera_position[:] = [1.0e8, 2.0e8, 3.0e8]
    v.grid_matrix3[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    v.current = s.epoch
    cnt, stt, fail = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1)
    ot, ox = np.zeros(10), np.zeros(30, np.float32)

    def call(rq, capacity):
        return L.eph_plot_points(eph._h, C.byref(v), 1, C.byref(rq), 0, None, None, None, capacity,
                                 ot.ctypes.data_as(C.POINTER(C.c_double)), ox.ctypes.data_as(C.POINTER(C.c_float)),
                                 cnt.ctypes.data_as(C.POINTER(C.c_int64)), stt.ctypes.data_as(C.POINTER(C.c_int32)),
                                 fail.ctypes.data_as(C.POINTER(C.c_double)))
    assert gpu.plot_points(eph, {"camera_position": (1.0, 2.0, 3.0), "current": s.epoch}, []) == []      # no plots: nothing to do
    assert call(gpu.PlotRequest(3, -1, 0, 0, s.epoch, s.epoch + 1.0, 0, 1, 1e-4, 100), 10) == gpu.ERR_BAD_ARGUMENT
    assert call(gpu.PlotRequest(s.n, -1, 0, 0, s.epoch, s.epoch + 1.0, 0, 1, 1e-4, 10), 10) == gpu.ERR_BAD_ARGUMENT
    assert call(gpu.PlotRequest(-1, -1, 0, 5, s.epoch, s.epoch + 1.0, 0, 1, 1e-4, 10), 10) == gpu.ERR_BAD_ARGUMENT   # no knots given
    assert call(gpu.PlotRequest(3, -1, 0, 0, s.epoch, s.epoch + 86400.0, 0, 1, 1e-4, 10), 10) == 0 and cnt[0] >= 2 and stt[0] == 0
    # a degenerate view (everything mapped onto the camera: the error estimate is NaN) makes the reference spin forever;
    # here the search gives up and says so
    v.grid_matrix3[:] = [0.0] * 9
    v.camera_position[:] = [0.0, 0.0, 0.0]
    assert call(gpu.PlotRequest(3, -1, 0, 0, s.epoch, s.epoch + 86400.0, 0, 1, 1e-4, 10), 10) == 0
    assert stt[0] == gpu.MAX_ITERATIONS_REACHED and cnt[0] == 1
