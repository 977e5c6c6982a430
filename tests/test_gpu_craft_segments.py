"""-m gpu: eph_craft_batch_plot_segments -- setup_segment_plotting (ephemeris_explorer/src/analysis.rs:159-296) composed on the device
from a batch's transition slabs and timelines, ending in the plot sampler -- against the Python restatement of
craft_segments_restatement.py (pinned on the CPU by test_craft_segments_abi.py) working from batch.events(c), pyoracle.timeline_new
and soi_parents, and, for the points, against eph_craft_batch_plot_points (itself pinned to the restatement of the sampler) fed with
requests built from the returned records. Every comparison is on bit patterns; there is no tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import craft_segments_restatement as R
from conftest import ROOT
from craft_cases import DAY, SHIP, perturbed, simple_system, snapshot_of_slabs  # noqa: F401  (the fixture)
from ephemeris_explorer_amd.systems import load_ship, soi_parents, soi_radii
from test_gpu_craft_plot import RES, assert_same_plots, views_for

pytestmark = pytest.mark.gpu

SEED = 20261018          # copies 4 and 5 miss the capture and leave Mars after the last burn: Flyby, Flyby Burn, Flyby (CPU oracle)


def config(start, end, **more):
    return {"start": start, "end": end, "tan2_angular_resolution": RES, "max_points_per_segment": 4000, **more}


def transitions_of(batch):
    counts = batch.event_counts()
    return {c: batch.events(c, counts)[0] for c in range(batch.n)}


def check(gpu, batch, view, configs, crafts, burns, parents, what):
    """one call against the restatement (records, out_first) and against plot_points (every row) -> (records, plots)"""
    crafts = np.asarray(crafts, dtype=np.int64)
    want, first = R.expected_segments(configs, crafts, transitions_of(batch), burns, parents)
    segments, plots = batch.plot_segments(view, configs, parents, craft=crafts)
    got = R.record_tuples(segments)
    assert R.same_records(got, want), (what, got[:3], want[:3], len(got), len(want))
    assert np.array_equal(np.searchsorted(segments["plot"], np.arange(len(configs) + 1)), first), what       # out_first, from the records
    only, none = batch.plot_segments(None, configs, parents, craft=crafts)
    assert none is None and only.tobytes() == segments.tobytes(), what
    if view is not None and len(segments):
        requests = R.requests_of(segments, lambda r: configs[int(r["plot"])])
        assert_same_plots(plots, batch.plot_points(view, requests, craft=crafts[segments["plot"]]), what)
        assert all(len(p[2]) == 0 and p[0] == 0 for r, p in zip(segments, plots) if r["start"] >= r["end"]), what
    return segments, plots


@pytest.fixture(scope="module")
def wave_case(gpu, simple_system):
    """6 craft to start + 215 d with events on: the ship, the ship without its last burn, four perturbed copies with all four burns"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    pos, vel = perturbed(ship, 6, SEED)
    pos[1], vel[1] = ship.pos, ship.vel
    full = ship.burn_tuples(s.names)
    burns = [full, full[:-1]] + [full] * 4
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), burns,
                                max_knots=8192).enable_events(soi_radii(s), 16, 8192)
    batch.propagate(ship.start + 215 * DAY)
    assert (batch.status()["status"] == 0).all() and (batch.event_counts()[2] == 0).all()
    return dict(batch=batch, burns=burns, parents=soi_parents(s), ship=ship, pos=pos, vel=vel)


def frame_configs(s, t0, last):
    """per craft: the whole window, [start + 100 d, start + 208 d], a window collapsed onto the craft's last transition, reference
    Sun, a disabled config, a window that ends before the first transition"""
    sun = s.names.index("Sun")
    return [config(t0, t0 + 400 * DAY), config(t0 + 100 * DAY, t0 + 208 * DAY), config(last, last),
            config(t0, t0 + 400 * DAY, reference_body=sun), config(t0, t0 + 400 * DAY, enabled=0, max_points_per_segment=100),
            config(t0 - 10 * DAY, t0 - DAY)]


def test_wave_form_records_and_points(gpu, simple_system, wave_case):
    """1. every window and reference on every craft, both views: records, out_first and every point row"""
    s, sol, eph, osol = simple_system
    batch, burns, parents, ship = (wave_case[k] for k in ("batch", "burns", "parents", "ship"))
    tr = transitions_of(batch)
    names = [[s.names[b] for b in tr[c][1]] for c in range(6)]
    assert names[0] == ["Earth", "Sun", "Mars"] and names[1] == ["Earth", "Sun", "Mars", "Sun"]
    configs, crafts = [], []
    for c in range(6):
        per = frame_configs(s, ship.start, float(tr[c][0][-1]))
        configs += per
        crafts += [c] * len(per)
    checked = 0
    for v, view in enumerate(views_for(s.epoch)):
        segments, plots = check(gpu, batch, view, configs, crafts, burns, parents, f"view {v}")
        checked += len(segments)
        per_entry = np.bincount(segments["plot"], minlength=len(configs)).reshape(6, 6)
        assert list(per_entry[0]) == [11, 4, 2, 11, 11, 0] and list(per_entry[1]) == [11, 3, 3, 10, 11, 0]
        kinds = set(int(k) for k in segments["kind"])
        assert {R.CAPTURE, R.ESCAPE, R.FLYBY, R.TRANSIT} <= kinds
        assert segments["overlapping"].any() and ((segments["kind"] == R.FLYBY) & (segments["is_burn"] == 1)).any()
        whole = segments[segments["plot"] % 6 == 0]                     # the whole window: every non-empty piece is drawn
        drawn = [len(plots[i][2]) for i in np.flatnonzero(segments["plot"] % 6 == 0)]
        assert all(n >= 2 for n, r in zip(drawn, whole) if r["start"] < min(r["end"], ship.start + 215 * DAY))
        off = segments[segments["plot"] % 6 == 4]                       # disabled: the records, nothing drawn
        assert len(off) == len(whole) and np.array_equal(off["kind"], whole["kind"])
        assert all(len(plots[i][2]) == 0 for i in np.flatnonzero(segments["plot"] % 6 == 4))
        assert not segments[segments["plot"] % 6 == 3]["overlapping"].any()          # reference Sun: no copy
        assert (segments[segments["plot"] % 6 == 2]["start"] >= segments[segments["plot"] % 6 == 2]["end"]).all()
        name = [gpu.segment_name(s.names, r) for r in segments[segments["plot"] == 6]]
        assert name == ["Earth Escape", "Earth Escape Burn", "Earth Escape", "Earth Escape Burn", "Earth Escape", "Sun Transit",
                        "Sun Transit Burn", "Sun Transit", "Mars Flyby", "Mars Flyby", "Sun Transit"]
    assert checked > 2 * 150                                            # no record is left unchecked (check() compares all of them)
    # one dict for all, craft == NULL
    segments, plots = batch.plot_segments(views_for(s.epoch)[0], config(ship.start, ship.start + 400 * DAY), parents)
    want, first = R.expected_segments([config(ship.start, ship.start + 400 * DAY)] * 6, range(6), tr, burns, parents)
    assert R.same_records(R.record_tuples(segments), want) and len(plots) == first[-1]


def test_orbit(gpu, simple_system):
    """2. three craft with the first burn only, one day: they stay at Earth -- Orbit, the burn piece dashed"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    pos, vel = perturbed(ship, 3, 7)
    burns = [ship.burn_tuples(s.names)[:1]] * 3
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), burns,
                                max_knots=4096).enable_events(soi_radii(s), 16, 1024)
    parents = soi_parents(s)
    cfg = [config(ship.start, ship.start + 400 * DAY)] * 3
    empty, nothing = batch.plot_segments(views_for(s.epoch)[1], cfg, parents)          # the search has not run: no transition, no plot
    assert len(empty) == 0 and nothing == []
    batch.propagate(ship.start + DAY)
    assert (batch.status()["status"] == 0).all()
    segments, plots = check(gpu, batch, views_for(s.epoch)[1], cfg, range(3), burns, parents, "orbit")
    assert len(segments) == 9 and (segments["kind"] == R.ORBIT).all() and list(segments["is_burn"]) == [0, 1, 0] * 3
    assert [gpu.segment_name(s.names, r) for r in segments[:3]] == ["Earth Orbit", "Earth Orbit Burn", "Earth Orbit"]
    assert all(len(p[2]) >= 2 for p in plots)


def test_the_lists_as_they_are_now(gpu, simple_system, wave_case):
    """3. after reset_events, after a restart of a subset, after reset_knots, on a clone"""
    s, sol, eph, osol = simple_system
    batch, burns, parents, ship = (wave_case[k] for k in ("batch", "burns", "parents", "ship"))
    view = views_for(s.epoch)[0]
    cfg = [config(ship.start, ship.start + 400 * DAY)] * 6
    before, before_plots = check(gpu, batch, view, cfg, range(6), burns, parents, "as propagated")
    again, again_plots = batch.clone().plot_segments(view, cfg, parents)
    assert again.tobytes() == before.tobytes()
    assert_same_plots(again_plots, before_plots, "clone")
    # only the newest transition: every record is Orbit
    a = batch.clone()
    a.reset_events()
    assert (a.event_counts()[0] == 1).all()
    segments, _ = check(gpu, a, view, cfg, range(6), burns, parents, "after reset_events")
    assert len(segments) and (segments["kind"] == R.ORBIT).all()
    # craft 0 and 2 restarted without their last burn: their records follow the new timeline and the new transitions
    b = batch.clone()
    sel = np.array([True, False, True, False, False, False])
    news = [bl[:-1] if sel[c] else bl for c, bl in enumerate(burns)]
    epoch, outcome = b.restart(news, which=sel)
    assert (outcome[sel] == 0).all()
    b.propagate(ship.start + 215 * DAY)
    assert (b.status()["status"] == 0).all()
    segments, _ = check(gpu, b, view, cfg, range(6), news, parents, "after restart")
    for c in range(6):
        same = segments[segments["plot"] == c].tobytes() == before[before["plot"] == c].tobytes()
        assert same == (not sel[c]), c
    assert segments[segments["plot"] == 0]["timeline_segment"].max() == 6           # three burns: seven pieces
    assert (segments[segments["plot"] == 0]["kind"] == R.FLYBY).any()               # the ship itself now flies by
    # a drained slab: the same records, the points cover only the drained slab's span
    d = batch.clone()
    last = np.array([d.knots(c)[0][-1] for c in range(6)])
    d.reset_knots()
    d.propagate(ship.start + 216 * DAY)
    segments, plots = check(gpu, d, view, cfg, range(6), burns, parents, "drained slab")
    if all(len(t[0]) == len(u[0]) for t, u in zip(transitions_of(d).values(), transitions_of(batch).values())):
        assert segments.tobytes() == before.tobytes()
    assert any(len(p[2]) for p in plots)
    assert all(p[2][0] >= last[int(r["plot"])] for r, p in zip(segments, plots) if len(p[2]))


_DEALT_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import ephemeris_explorer_amd as ea
import craft_segments_restatement as R
from craft_cases import DAY, SHIP, perturbed
from test_gpu_craft_plot import RES, assert_same_plots, views_for
from ephemeris_explorer_amd.systems import load_system, load_ship, parse_epoch, soi_parents, soi_radii
s = load_system(sys.argv[1] + "/tests/golden/systems/simple_solar_system_2433282.5")
ship = load_ship(SHIP)
eph = ea.Ephemeris(ea.NBodyPropagator.from_system(s).propagate(parse_epoch("1951-01-01 00:00:00")), s.mu)
n = 192
pos, vel = perturbed(ship, n, 20261018)
full = ship.burn_tuples(s.names)
burns = [(full, full[:-1], full[:1])[c % 3] for c in range(n)]
batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, ea.AdaptiveParams.default(ship.tolerance), burns,
                           max_knots=8192).enable_events(soi_radii(s), 16, 8192)
batch.propagate(ship.start + 215 * DAY)
st = batch.status()["status"]
assert np.isin(st, (0, ea.KNOTS_FULL)).all() and (st == 0).sum() >= n // 3, st
parents = soi_parents(s)
counts = batch.event_counts()
tr = {c: batch.events(c, counts)[0] for c in range(n)}
view = views_for(s.epoch)[0]
cfg = {"start": ship.start, "end": ship.start + 400 * DAY, "tan2_angular_resolution": RES, "max_points_per_segment": 512}
rng = np.random.default_rng(5)
kinds = set()
for crafts in (None, np.concatenate([rng.permutation(n), rng.integers(0, n, 40), [7, 7, 7]])):
    listed = np.arange(n) if crafts is None else crafts
    want, first = R.expected_segments([cfg] * len(listed), listed, tr, burns, parents)
    segments, plots = batch.plot_segments(view, cfg if crafts is None else [cfg] * len(listed), parents, craft=crafts)
    assert R.same_records(R.record_tuples(segments), want), (len(segments), len(want))
    assert np.array_equal(np.searchsorted(segments["plot"], np.arange(len(listed) + 1)), first)
    requests = R.requests_of(segments, lambda r: cfg)
    assert_same_plots(plots, batch.plot_points(view, requests, craft=listed[segments["plot"]]), "dealt lanes")
    assert sum(len(p[2]) >= 2 for p in plots) > len(plots) // 2
    kinds |= set(int(k) for k in segments["kind"])
assert kinds == {0, 1, 2, 3, 4}, kinds
print("dealt lanes ok", len(segments))
'''


def test_dealt_lanes(gpu):
    """4. the thread form (forced in a child process: the form is read once per process): 192 craft whose burn lists differ from craft
    to craft, dealt to the lanes; craft == NULL and a shuffled craft list with repeats, records against the restatement and points
    against plot_points with the same requests"""
    env = dict(os.environ, EPH_CRAFT_FORM="thread")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _DEALT_SCRIPT, str(ROOT)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0 and "dealt lanes ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_the_batch_is_untouched(gpu, simple_system, wave_case):
    """5. summary, knot slabs and events are bit-equal before and after; a following propagate equals a twin's that never plotted"""
    s, sol, eph, osol = simple_system
    batch, burns, parents, ship = (wave_case[k] for k in ("batch", "burns", "parents", "ship"))
    a, twin = batch.clone(), batch.clone()
    before = snapshot_of_slabs(a)
    cfg = frame_configs(s, ship.start, ship.start + 206 * DAY) * 6
    segments, plots = a.plot_segments(views_for(s.epoch)[1], cfg, parents, craft=np.repeat(np.arange(6), 6))
    assert len(segments) and any(len(p[2]) for p in plots)
    assert snapshot_of_slabs(a) == before == snapshot_of_slabs(twin)
    a.propagate(ship.start + 217 * DAY)
    twin.propagate(ship.start + 217 * DAY)
    assert snapshot_of_slabs(a) == snapshot_of_slabs(twin)


def test_sizing_and_refusals(gpu, simple_system, wave_case):
    """6. the records-only call, a record array one short, every refusal: poisoned buffers stay poisoned"""
    s, sol, eph, osol = simple_system
    batch, burns, parents, ship = (wave_case[k] for k in ("batch", "burns", "parents", "ship"))
    L, h = batch._L, batch._h
    dp, fp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    n, cap = 6, 16
    view = gpu.PlotView()
    view.camera_position[:] = [1.2e8, -3.0e8, 2.0e8]
    view.grid_matrix3[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    view.current = s.epoch + 30 * DAY
    whole = (ship.start, ship.start + 400 * DAY)
    expected, _ = batch.plot_segments(None, config(*whole), parents)
    total = len(expected)
    assert total == len(R.expected_segments([config(*whole)] * n, range(n), transitions_of(batch), burns, parents)[0]) and total >= 6 * 11
    rows = total + 2
    seg = np.full(rows * 56, 0xA5, np.uint8)
    first = np.full(n + 1, -99, np.int64)
    ot, ox = np.full(rows * cap, -7.25), np.full(rows * cap * 3, -7.25, dtype=np.float32)
    cnt, stt, fail = np.full(rows, -99, np.int64), np.full(rows, -99, np.int32), np.full(rows, -7.25)
    outs = [ot.ctypes.data_as(dp), ox.ctypes.data_as(fp), cnt.ctypes.data_as(i64p), stt.ctypes.data_as(i32p), fail.ctypes.data_as(dp)]

    def poisoned(but_first=False):
        return ((seg == 0xA5).all() and (but_first or (first == -99).all()) and (ot == -7.25).all() and (ox == np.float32(-7.25)).all() and
                (cnt == -99).all() and (stt == -99).all() and (fail == -7.25).all())

    def one(start=whole[0], end=whole[1], bound=0, max_points=cap, ref=-1):
        return gpu.OrbitPlotConfig(start, end, bound, 1, RES, max_points, ref)

    def call(cfgs, n_plots=None, craft=None, par=parents, scap=rows, records=True, fst=True, vw=view, capacity=cap, o=outs, handle=h):
        arr = (gpu.OrbitPlotConfig * max(len(cfgs), 1))(*cfgs) if cfgs is not None else None
        cr = None if craft is None else np.asarray(craft, dtype=np.int64)
        pa = None if par is None else np.ascontiguousarray(par, dtype=np.int32)
        return L.eph_craft_batch_plot_segments(handle, len(cfgs) if n_plots is None else n_plots, arr,
                                               None if cr is None else cr.ctypes.data_as(i64p), None if pa is None else pa.ctypes.data_as(i32p),
                                               scap, seg.ctypes.data_as(C.POINTER(gpu.PlotSegment)) if records else None,
                                               first.ctypes.data_as(i64p) if fst else None, None if vw is None else C.byref(vw), capacity, *o)
    bad = gpu.ERR_BAD_ARGUMENT
    ok = [one()] * n
    assert call(ok, handle=None) == bad
    assert call(ok, n_plots=-1) == bad and call(None, n_plots=1) == bad
    assert call(ok, par=None) == bad and call(ok, fst=False) == bad
    assert call(ok, scap=-1) == bad and call(ok, records=False) == bad
    assert call(ok[:1], craft=[n]) == bad and call(ok[:1], craft=[-1]) == bad
    assert call(ok + ok[:1]) == bad                                     # craft == NULL: at most one entry per craft
    assert call([one(ref=-2)]) == bad and call([one(ref=s.n)]) == bad
    for b, p in ((0, -2), (0, s.n), (3, 3)):
        wrong = parents.copy()
        wrong[b] = p
        assert call(ok, par=wrong) == bad
    assert call([one(start=float("nan"))]) == bad and call([one(end=float("nan"))]) == bad
    assert call([one(bound=3)]) == bad and call([one(bound=-1)]) == bad
    assert call([one(max_points=-1)]) == bad and call([one(), one(bound=3)]) == bad
    # with a view: the point-output and capacity rules of eph_craft_batch_plot_points
    assert call(ok, capacity=-1) == bad and call([one(max_points=cap + 1)]) == bad
    for k in (2, 3, 4):
        assert call(ok, o=outs[:k] + [None] + outs[k + 1:]) == bad
    assert call(ok, o=[None] + outs[1:]) == bad and call(ok, o=outs[:1] + [None] + outs[2:]) == bad
    plain = gpu.SpacecraftBatch(eph, ship.start, wave_case["pos"], wave_case["vel"], "Verner87", max_knots=64)     # no events
    assert call(ok, handle=plain._h) == bad
    assert call([], n_plots=0) == 0 and call(None, n_plots=0, par=None, records=False, scap=0, fst=False, o=[None] * 5) == 0
    assert poisoned()
    # one record short: the needed total comes back in out_first, nothing else is written
    assert call(ok, scap=total - 1) == bad
    assert first[n] == total and list(first) == list(np.searchsorted(expected["plot"], np.arange(n + 1))) and poisoned(but_first=True)
    first[:] = -99
    assert call(ok, scap=0, records=False, vw=None, o=[None] * 5) == bad and first[n] == total and poisoned(but_first=True)   # the sizing call
    # records only: view == NULL ignores the point arguments
    assert call(ok, vw=None, capacity=-1, o=[None] * 5) == 0
    assert seg[:total * 56].tobytes() == expected.tobytes() and (seg[total * 56:] == 0xA5).all()
    assert (ot == -7.25).all() and (cnt == -99).all() and (stt == -99).all() and (fail == -7.25).all()
    # the drawing call gives the same records; rows beyond the total and entries beyond a row's count stay as they were
    seg[:] = 0xA5
    assert call(ok) == 0
    assert seg[:total * 56].tobytes() == expected.tobytes() and (seg[total * 56:] == 0xA5).all()
    assert (cnt[:total] >= 0).all() and (cnt[:total] <= cap).all() and (cnt[:total] >= 2).any() and (stt[:total] == 0).all()
    assert (cnt[total:] == -99).all() and (stt[total:] == -99).all() and (ot[total * cap:] == -7.25).all()
    assert all((ot[r * cap + cnt[r]:(r + 1) * cap] == -7.25).all() for r in range(total))
