"""CPU: eph_craft_batch_plot_markers (the app's plot_*_markers and *_marker_picking for ships that live in a batch) is part of the
boundary -- declared, exported, bound, wrapped -- and refuses a missing batch before it touches a device; the Python restatement the
GPU test compares against (craft_markers_restatement.py) is pinned here on the Mars-transfer ship in the C oracle, against record
lists worked out by hand from the ship's transitions, burns and apsides. What the call computes is checked on the GPU
(test_gpu_craft_markers.py)."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import craft_markers_restatement as R
from conftest import ROOT, SYSTEMS, load_system
from ephemeris_explorer_amd.systems import load_ship, parse_epoch, soi_radii
from oracle import orc

DAY = 86400.0
REQUEST_FIELDS = ["int32_t reference_body", "int32_t kinds", "double first, last"]
MARKER_FIELDS = ["int64_t request", "int32_t kind", "int32_t index", "int32_t body", "int32_t status", "double time", "double position[3]",
                 "double distance", "double apsis_distance", "double frame[9]"]
ARGS = ["eph_craft_batch *b", "int64_t n_requests", "const eph_marker_request *requests", "const int64_t *craft",
        "int64_t marker_capacity", "eph_plot_marker *out_markers", "int64_t *out_first"]


def test_plot_markers_is_declared_exported_bound_and_wrapped(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, want in (("eph_marker_request", REQUEST_FIELDS), ("eph_plot_marker", MARKER_FIELDS)):
        m = re.search(rf"typedef\s+struct\s+{name}\s*\{{([^}}]*)\}}\s*{name}\s*;", code)
        assert m, f"include/ephemeris_amd.h does not declare {name}"
        assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == want
    m = re.search(r"int32_t\s+eph_craft_batch_plot_markers\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_plot_markers"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert "eph_craft_batch_plot_markers" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_plot_markers")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(getattr(product_lib.SpacecraftBatch, "plot_markers"))
    assert callable(product_lib.marker_requests) and callable(product_lib.marker_name)
    assert C.sizeof(product_lib.MarkerRequest) == 24 and C.sizeof(product_lib.PlotMarker) == 144          # the C layouts
    assert [f[0] for f in product_lib.MarkerRequest._fields_] == ["reference_body", "kinds", "first", "last"]
    assert [f[0] for f in product_lib.PlotMarker._fields_] == list(R.FIELDS)
    dt = product_lib.SpacecraftBatch.MARKER                          # the record array is the C struct, field for field
    assert dt.itemsize == 144 and [(n, dt.fields[n][1]) for n in dt.names] == [
        (n, getattr(product_lib.PlotMarker, n).offset) for n, _ in product_lib.PlotMarker._fields_]
    assert dt["position"].shape == (3,) and dt["frame"].shape == (9,)
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "plot_markers" in hpp and "eph_craft_batch_plot_markers" in hpp
    assert product_lib.marker_name(["Sun", "Mars"], {"kind": 2, "body": 1}) == "Mars Periapsis"
    assert product_lib.marker_name(["Sun", "Mars"], {"kind": 1, "body": 0}) == "Sun Transition"
    assert product_lib.marker_name(["Sun", "Mars"], {"kind": 0, "body": -1}) == "Inertial Manoeuvre"
    assert product_lib.marker_name(["Sun", "Mars"], {"kind": 5, "body": -1}) == "End"


def test_marker_requests_follows_the_plots(product_lib):
    """kinds = 4 | 8 | (1 if is_burn) | (2 if not overlapping), first / last from the plot's epoch row, 0 for a plot without points"""
    segments = np.zeros(4, dtype=product_lib.SpacecraftBatch.SEGMENT)
    segments["reference_body"] = [3, 0, 5, 3]
    segments["is_burn"] = [0, 1, 0, 1]
    segments["overlapping"] = [0, 0, 1, 0]
    rows = [np.array([1.0, 2.0, 4.0]), np.array([4.0, 5.0]), np.array([7.0]), np.zeros(0)]
    plots = [(0, 0.0, t, np.zeros((len(t), 3), dtype=np.float32)) for t in rows]
    assert product_lib.marker_requests(segments, plots) == [
        {"reference_body": 3, "kinds": 4 | 8 | 2, "first": 1.0, "last": 4.0}, {"reference_body": 0, "kinds": 4 | 8 | 1 | 2, "first": 4.0, "last": 5.0},
        {"reference_body": 5, "kinds": 4 | 8, "first": 7.0, "last": 7.0}, {"reference_body": 3, "kinds": 0, "first": 0.0, "last": 0.0}]


def test_craft_markers_example_compiles_and_links(product_lib, tmp_path):
    """examples/craft_markers.cpp against the product alone, warning-free (the flags of its siblings); without a device its first
    compute call throws Error{EPH_ERR_NO_DEVICE} (exit 77)."""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_markers_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_markers.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if product_lib.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "Manoeuvre" in r.stdout and "Periapsis" in r.stdout and "Transition" in r.stdout, (r.stdout, r.stderr)


def test_a_null_batch_is_refused_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing batch whatever the other arguments, before any device work (this machine may have no
    device at all), and nothing is written into the caller's buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    i64p = C.POINTER(C.c_int64)
    req = (product_lib.MarkerRequest * 2)(product_lib.MarkerRequest(-1, 15, 0.0, 86400.0), product_lib.MarkerRequest(0, 12, 0.0, 86400.0))
    craft = np.array([0, 1], dtype=np.int64)
    marks = np.full(4 * 144, 0xA5, np.uint8)
    first = np.full(3, -99, np.int64)
    records = marks.ctypes.data_as(C.POINTER(product_lib.PlotMarker))
    calls = 0
    for (n, requests), cr, (cap, recs), fst in itertools.product(
            ((2, req), (1, req), (0, None), (-1, None), (2, None)), (None, craft.ctypes.data_as(i64p)),
            ((4, records), (0, None), (-1, records), (4, None)), (None, first.ctypes.data_as(i64p))):
        assert L.eph_craft_batch_plot_markers(None, n, requests, cr, cap, recs, fst) == bad
        calls += 1
    assert calls == 5 * 2 * 4 * 2
    assert (marks == 0xA5).all() and (first == -99).all()


@pytest.fixture(scope="module")
def mars_ship():
    """the simple system to 1952-01-01 in the C oracle, the Mars-transfer ship to start + 215 d with its events and knots"""
    s = load_system("simple_solar_system_2433282.5")
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    assert o.step_to(parse_epoch("1952-01-01 00:00:00")) == 0
    osol = o.take_solution()
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    burns = ship.burn_tuples(s.names)
    c = orc.Craft(osol, s.mu, ship.start, ship.pos, ship.vel, ship.integrator, tol_pos=ship.tolerance, tol_vel=ship.tolerance,
                  burns=burns, soi_radius=soi_radii(s))
    assert c.step_to(ship.start + 215 * DAY) == 0
    return s, osol, ship, burns, (c.transitions(), c.apsides()), c.knots()


def test_the_restatement_gives_the_ships_marker_lists(mars_ship):
    """The Mars-transfer ship to start + 215 d: transitions at days 0.0 (Earth), 2.499 (Sun) and 206.015 (Mars), burns starting at
    days 0.011, 0.030, 58.175 and 207.656, all in relative frames, 94 apsides, the first two an apoapsis (7000.0 km) and a periapsis
    at days 0.0 and 0.030. Under kinds = 15, first = t0 and last = the second transition's epoch: 2 manoeuvres, 2 transitions (both
    ends are inclusive), 2 apsides, Start, no End, in this order; every smaller mask selects the matching subset; first > last gives
    nothing.

    The first apsis: its epoch is not t0 itself but t0 + 0.0036621 s -- the bisection of find_root_bisection stops at a bracket
    narrower than 1e-3 s and returns its left end, which the radial velocity's sign change at the start leaves just after t0. So the
    window collapsed onto t0 keeps the transition and Start, whose epochs ARE t0, and not that apsis (t0 < its epoch); the edges
    time == first and time == first == last on an apsis are pinned with windows placed on the apsis's own epoch.

    With reference_body = Earth the first apsis's distance equals its stored apsis_distance bit for bit in the CPU oracle
    (7000.00004618917 km both: the search stores distance_at at the same epoch from the same two positions), and that is asserted."""
    s, osol, ship, burns, events, knots = mars_ship
    (tr_t, tr_b), (ap_t, ap_d, ap_b, ap_k) = events
    sun, earth, mars = (s.names.index(x) for x in ("Sun", "Earth", "Mars"))
    t0 = ship.start
    assert [s.names[b] for b in tr_b] == ["Earth", "Sun", "Mars"]
    assert [round((t - t0) / DAY, 3) for t in tr_t] == [0.0, 2.499, 206.015] and tr_t[0] == t0
    assert [round((b[0] - t0) / DAY, 3) for b in burns] == [0.011, 0.03, 58.175, 207.656] and all(b[3] >= 0 for b in burns)
    assert len(ap_t) == 94 and [round((t - t0) / DAY, 3) for t in ap_t[:2]] == [0.0, 0.03] and list(ap_k[:2]) == [1, 0]
    assert round(float(ap_d[0]), 1) == 7000.0 and 0.0 < ap_t[0] - t0 < 1e-2
    assert knots[0][0] == t0 and knots[0][-1] >= t0 + 215 * DAY

    def lists(kinds, first, last, reference=earth):
        return R.markers_of(0, {"reference_body": reference, "kinds": kinds, "first": first, "last": last}, events, knots, burns, osol)

    second = float(tr_t[1])
    full = lists(15, t0, second)
    M, T, P, A, S = R.MANOEUVRE, R.TRANSITION, R.PERIAPSIS, R.APOAPSIS, R.START
    assert [m[1] for m in full] == [M, M, T, T, A, P, S]
    assert [m[2] for m in full] == [1, 3, 0, 1, 0, 1, 0]             # timeline pieces 1 and 3 are the burns; list indices; 0 for a bound
    assert [m[3] for m in full] == [burns[0][3], burns[1][3], earth, sun, earth, earth, -1]
    assert [m[5] for m in full] == [burns[0][0], burns[1][0], t0, second, float(ap_t[0]), float(ap_t[1]), t0]
    assert full[2][5] == t0 and full[3][5] == second                 # time == first and time == last: both ends inclusive
    assert [m[4] for m in full] == [3, 3, 1, 1, 1, 1, 1]             # every position is Some, both frames are
    assert all(m[8] == 0.0 and m[9] == R.ZERO9 for m in full[2:4] + full[6:]) and all(m[9] != R.ZERO9 for m in full[:2])
    assert [m[8] for m in full[4:6]] == [float(ap_d[0]), float(ap_d[1])]
    for frame in (m[9] for m in full[:2]):                           # an orthonormal right-handed TNB: x, z, y with z = x cross y
        x, z, y = frame[:3], frame[3:6], frame[6:]
        assert all(abs(R.length(v) - 1.0) < 1e-15 for v in (x, y, z))
        assert max(abs(a - b) for a, b in zip(R.cross(x, y), z)) < 1e-15
    assert R.bits(full[4][7]) == R.bits(full[4][8])                  # the first apsis: distance == the stored distance, by bits
    assert full[6][6] == full[2][6] and full[6][7] == full[2][7]     # Start and the transition at t0: the same position
    # every smaller mask selects the matching subset
    group = {M: 1, T: 2, P: 4, A: 4, S: 8, R.END: 8}
    for kinds in range(16):
        assert R.same_markers(lists(kinds, t0, second), [m for m in full if group[m[1]] & kinds]), kinds
    # collapsed windows: on t0 the transition and Start; on the first apsis's epoch that apsis alone
    assert [m[1] for m in lists(15, t0, t0)] == [T, S]
    assert [(m[1], m[2]) for m in lists(15, float(ap_t[0]), float(ap_t[0]))] == [(A, 0)]
    # time == first on an apsis: the window from its epoch on leaves out what lies at t0
    assert [(m[1], m[2]) for m in lists(15, float(ap_t[0]), second)] == [(M, 1), (M, 3), (T, 1), (A, 0), (P, 1)]
    assert lists(15, second, t0) == [] and lists(15, t0 + DAY, t0) == []          # first > last: nothing
    # the whole span: all of it, End at the last knot
    whole = lists(15, t0, float(knots[0][-1]), reference=-1)
    assert len(whole) == 4 + 3 + 94 + 2 and whole[-1][1] == R.END and whole[-1][5] == knots[0][-1] and all(m[4] & 1 for m in whole)
    assert sum(m[1] == P for m in whole) + sum(m[1] == A for m in whole) == 94
    # a window before the flight finds no candidate at all
    assert lists(15, t0 - 10 * DAY, t0 - DAY) == []
    # without events: manoeuvres and bounds only
    plain = R.markers_of(0, {"reference_body": earth, "kinds": 15, "first": t0, "last": second}, R.NO_EVENTS, knots, burns, osol)
    assert R.same_markers(plain, [m for m in full if m[1] in (M, S)])


def test_same_markers_compares_bits():
    a = (0, 2, 1, 3, 1, 5.0, (1.0, 2.0, 3.0), 4.0, 4.0, R.ZERO9)
    assert R.same_markers([a], [a])
    assert not R.same_markers([a], [a[:6] + ((1.0, 2.0, -0.0 + 3.0000000000000004),) + a[7:]])
    assert not R.same_markers([a], [a[:9] + ((-0.0,) + (0.0,) * 8,)])           # -0.0 is not +0.0
    assert not R.same_markers([a], [a, a]) and not R.same_markers([a], [(1,) + a[1:]])
