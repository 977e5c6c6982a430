"""CPU: eph_craft_batch_plot_segments (the app's setup_segment_plotting for ships that live in a batch) is part of the boundary --
declared, exported, bound, wrapped -- and refuses a missing batch before it touches a device; soi_parents and the Python restatement
the GPU test compares against (craft_segments_restatement.py) are pinned here against the record lists the Mars-transfer ship must
give, from the C oracle's transitions. What the call computes is checked on the GPU (test_gpu_craft_segments.py)."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import craft_segments_restatement as R
from conftest import ROOT, SYSTEMS, load_system
from ephemeris_explorer_amd.systems import load_ship, parse_epoch, soi_parents, soi_radii
from oracle import orc

DAY = 86400.0
CONFIG_FIELDS = ["double start, end", "int32_t bound", "int32_t enabled", "double tan2_angular_resolution",
                 "int64_t max_points_per_segment", "int32_t reference_body"]
SEGMENT_FIELDS = ["int64_t plot", "int32_t transition", "int32_t timeline_segment", "int32_t soi_body", "int32_t reference_body",
                  "int32_t kind", "int32_t is_burn", "int32_t overlapping", "double start, end"]
ARGS = ["eph_craft_batch *b", "int64_t n_plots", "const eph_orbit_plot_config *configs", "const int64_t *craft",
        "const int32_t *body_parent", "int64_t segment_capacity", "eph_plot_segment *out_segments", "int64_t *out_first",
        "const eph_plot_view *view", "int64_t capacity", "double *out_t", "float *out_xyz", "int64_t *out_count", "int32_t *out_status",
        "double *out_failed_at"]


def test_plot_segments_is_declared_exported_bound_and_wrapped(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, want in (("eph_orbit_plot_config", CONFIG_FIELDS), ("eph_plot_segment", SEGMENT_FIELDS)):
        m = re.search(rf"typedef\s+struct\s+{name}\s*\{{([^}}]*)\}}\s*{name}\s*;", code)
        assert m, f"include/ephemeris_amd.h does not declare {name}"
        assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == want
    m = re.search(r"int32_t\s+eph_craft_batch_plot_segments\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_plot_segments"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert "eph_craft_batch_plot_segments" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_plot_segments")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(getattr(product_lib.SpacecraftBatch, "plot_segments")) and callable(product_lib.segment_name)
    assert C.sizeof(product_lib.OrbitPlotConfig) == 48 and C.sizeof(product_lib.PlotSegment) == 56      # the C layouts
    assert [f[0] for f in product_lib.OrbitPlotConfig._fields_] == [
        "start", "end", "bound", "enabled", "tan2_angular_resolution", "max_points_per_segment", "reference_body"]
    assert [f[0] for f in product_lib.PlotSegment._fields_] == list(R.FIELDS)
    dt = product_lib.SpacecraftBatch.SEGMENT                         # the record array is the C struct, field for field
    assert dt.itemsize == 56 and [(n, dt.fields[n][1]) for n in dt.names] == [
        (n, getattr(product_lib.PlotSegment, n).offset) for n, _ in product_lib.PlotSegment._fields_]
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "plot_segments" in hpp and "eph_craft_batch_plot_segments" in hpp
    assert product_lib.segment_name(["Sun", "Mars"], {"soi_body": 1, "kind": 2, "is_burn": 1}) == "Mars Flyby Burn"
    assert product_lib.segment_name(["Sun", "Mars"], {"soi_body": 0, "kind": 3, "is_burn": 0}) == "Sun Transit"


def test_craft_segments_example_compiles_and_links(product_lib, tmp_path):
    """examples/craft_segments.cpp against the product alone, warning-free (the flags of its siblings); without a device its first
    compute call throws Error{EPH_ERR_NO_DEVICE} (exit 77)."""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_segments_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_segments.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if product_lib.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "Flyby" in r.stdout and "Capture" in r.stdout, (r.stdout, r.stderr)


def test_a_null_batch_is_refused_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing batch whatever the other arguments, before any device work (this machine may have no
    device at all), and nothing is written into the caller's buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    dp, fp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    cfg = (product_lib.OrbitPlotConfig * 2)(product_lib.OrbitPlotConfig(0.0, 86400.0, 0, 1, 1e-4, 8, -1),
                                            product_lib.OrbitPlotConfig(0.0, 86400.0, 0, 1, 1e-4, 8, 0))
    craft = np.array([0, 1], dtype=np.int64)
    parents = np.array([-1, 0, 0], dtype=np.int32)
    seg = np.full(4 * 56, 0xA5, np.uint8)
    first = np.full(3, -99, np.int64)
    ot, ox = np.full(4 * 8, -7.25), np.full(4 * 8 * 3, -7.25, dtype=np.float32)
    cnt, st, fail = np.full(4, -99, np.int64), np.full(4, -99, np.int32), np.full(4, -7.25)
    view = product_lib.PlotView()
    points = (8, ot.ctypes.data_as(dp), ox.ctypes.data_as(fp), cnt.ctypes.data_as(i64p), st.ctypes.data_as(i32p), fail.ctypes.data_as(dp))
    records = seg.ctypes.data_as(C.POINTER(product_lib.PlotSegment))
    calls = 0
    for (n, configs), cr, par, (scap, recs), fst, vw, pts in itertools.product(
            ((2, cfg), (1, cfg), (0, None), (-1, None), (2, None)), (None, craft.ctypes.data_as(i64p)), (None, parents.ctypes.data_as(i32p)),
            ((4, records), (0, None), (-1, records)), (None, first.ctypes.data_as(i64p)), (None, C.byref(view)),
            (points, (0, None, None, None, None, None))):
        assert L.eph_craft_batch_plot_segments(None, n, configs, cr, par, scap, recs, fst, vw, *pts) == bad
        calls += 1
    assert calls == 5 * 2 * 2 * 3 * 2 * 2 * 2
    assert (seg == 0xA5).all() and (first == -99).all() and (ot == -7.25).all() and (ox == np.float32(-7.25)).all()
    assert (cnt == -99).all() and (st == -99).all() and (fail == -7.25).all()


@pytest.fixture(scope="module")
def mars_ship():
    """the simple system to 1952-01-01 in the C oracle, the Mars-transfer ship with its sphere radii"""
    s = load_system("simple_solar_system_2433282.5")
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    assert o.step_to(parse_epoch("1952-01-01 00:00:00")) == 0
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    return s, o.take_solution(), ship, soi_radii(s)


def test_soi_parents_of_the_simple_system():
    s = load_system("simple_solar_system_2433282.5")
    parents = soi_parents(s)
    assert parents.dtype == np.int32 and len(parents) == s.n
    sun, earth, moon = (s.names.index(x) for x in ("Sun", "Earth", "Moon"))
    assert parents[sun] == -1 and parents[moon] == earth
    assert all(parents[b] == sun for b in range(s.n) if b not in (sun, moon))


def test_the_restatement_gives_the_ships_record_lists(product_lib, mars_ship):
    """The Mars-transfer ship with all four burns, without its last burn and with its first burn only, under the whole window, the
    window [start + 100 d, start + 208 d], reference Sun and a window collapsed onto the last transition: kinds, burns, overlapping
    copies and references as setup_segment_plotting spawns them (worked out by hand from the transitions)."""
    s, osol, ship, soi = mars_ship
    parents = soi_parents(s)
    sun, earth, mars = (s.names.index(x) for x in ("Sun", "Earth", "Mars"))
    burns = ship.burn_tuples(s.names)
    assert len(burns) == 4
    t0 = ship.start
    whole = {"start": t0, "end": t0 + 400 * DAY}

    def lists(burn_list, days, config):
        c = orc.Craft(osol, s.mu, t0, ship.pos, ship.vel, ship.integrator, tol_pos=ship.tolerance, tol_vel=ship.tolerance,
                      burns=burn_list, soi_radius=soi)
        assert c.step_to(t0 + days * DAY) == 0
        tr = c.transitions()
        records, first = R.expected_segments([config], [0], {0: tr}, {0: burn_list}, parents)
        assert list(first) == [0, len(records)] and all(r[0] == 0 for r in records)
        names = [product_lib.segment_name(s.names, dict(zip(R.FIELDS, r))) for r in records]
        return tr, records, names

    escape = ["Earth Escape", "Earth Escape Burn", "Earth Escape", "Earth Escape Burn", "Earth Escape"]
    transit = ["Sun Transit", "Sun Transit Burn", "Sun Transit"]
    # all four burns: Earth, Sun (day 2.499), Mars (day 206.015)
    tr, records, names = lists(burns, 215, whole)
    assert [s.names[b] for b in tr[1]] == ["Earth", "Sun", "Mars"]
    assert [round((t - t0) / DAY, 3) for t in tr[0]] == [0.0, 2.499, 206.015]
    assert names == escape + transit + ["Mars Capture", "Mars Capture Burn", "Mars Capture"]
    assert [r[5] for r in records] == [R.ESCAPE] * 5 + [R.TRANSIT] * 3 + [R.CAPTURE] * 3
    assert [r[4] for r in records] == [earth] * 5 + [sun] * 3 + [mars] * 3 and not any(r[7] for r in records)
    assert [r[1] for r in records] == [0] * 5 + [1] * 3 + [2] * 3 and [r[2] for r in records] == [0, 1, 2, 3, 4, 4, 5, 6, 6, 7, 8]
    assert records[0][8] == t0 and records[4][9] == tr[0][1] == records[5][8] and records[-1][9] == whole["end"]
    assert all(r[8] < r[9] for r in records)
    # the window [start + 100 d, start + 208 d]
    _, records, names = lists(burns, 215, {"start": t0 + 100 * DAY, "end": t0 + 208 * DAY})
    assert names == ["Sun Transit", "Mars Capture", "Mars Capture Burn", "Mars Capture"]
    assert records[0][8] == t0 + 100 * DAY and records[-1][9] == t0 + 208 * DAY
    # reference Sun: every record relative to the Sun
    _, records, _ = lists(burns, 215, {**whole, "reference_body": sun})
    assert len(records) == 11 and all(r[4] == sun and r[7] == 0 for r in records)
    # a window collapsed onto the last transition's epoch: every record empty
    _, records, names = lists(burns, 215, {"start": tr[0][-1], "end": tr[0][-1]})
    assert names == ["Sun Transit", "Mars Capture"] and all(r[8] >= r[9] for r in records)
    # a window that ends before the first transition: nothing
    assert lists(burns, 215, {"start": t0 - 10 * DAY, "end": t0 - DAY})[1] == []
    # without the last burn the ship leaves Mars again (day 209.298): a flyby, drawn a second time relative to the Sun
    tr, records, names = lists(burns[:-1], 215, whole)
    assert [s.names[b] for b in tr[1]] == ["Earth", "Sun", "Mars", "Sun"] and round((tr[0][3] - t0) / DAY, 3) == 209.298
    assert names == escape + transit + ["Mars Flyby", "Mars Flyby", "Sun Transit"]
    assert [(r[4], r[7]) for r in records[8:]] == [(mars, 0), (sun, 1), (sun, 0)]
    assert records[8][8:] == records[9][8:] == (tr[0][2], tr[0][3])
    _, records, names = lists(burns[:-1], 215, {**whole, "reference_body": sun})
    assert names == escape + transit + ["Mars Flyby", "Sun Transit"] and not any(r[7] for r in records)
    # the first burn only: the ship stays at Earth
    tr, records, names = lists(burns[:1], 1, whole)
    assert [s.names[b] for b in tr[1]] == ["Earth"]
    assert names == ["Earth Orbit", "Earth Orbit Burn", "Earth Orbit"] and [r[5] for r in records] == [R.ORBIT] * 3
    assert [r[6] for r in records] == [0, 1, 0]


def test_segments_between_is_two_lower_bounds():
    """Timeline::segments_between on a timeline with a burn: the piece that ends AT start is left out, the piece that starts AT end
    too; an inverted window gives an empty or inverted range (the reference's slice panics on the latter)"""
    from oracle import pyoracle as po
    tl = po.timeline_new([(10.0, 20.0, (1.0, 0.0, 0.0), -1), (30.0, 40.0, (1.0, 0.0, 0.0), -1)])
    assert len(tl) == 5
    assert R.segments_between(tl, 0.0, 100.0) == (0, 5)
    assert R.segments_between(tl, 10.0, 20.0) == (1, 2)
    assert R.segments_between(tl, 10.0, 20.5) == (1, 3)
    assert R.segments_between(tl, 15.0, 15.0) == (1, 2)
    assert R.segments_between(tl, 20.0, 20.0) == (2, 2)
    lo, hi = R.segments_between(tl, 35.0, 15.0)
    assert lo > hi
