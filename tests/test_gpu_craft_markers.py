"""-m gpu: eph_craft_batch_plot_markers -- the markers the app draws on, and picks from, a ship's plots (ephemeris_explorer/src/ui/world/
tooltip.rs:84-245, picking.rs:256-447), counted and evaluated on the device from a batch's timeline CSR, event slabs, knot slabs and
the live table -- against the Python restatement of craft_markers_restatement.py (pinned on the CPU by test_craft_markers_abi.py)
working from batch.events(c), batch.knots(c), the burn tuples and the oracle's solution, and, for the positions, against
eph_craft_batch_eval at the markers' epochs. Every comparison is on bit patterns; there is no tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import craft_markers_restatement as R
from conftest import ROOT, load_system
from craft_cases import DAY, SHIP, bits, perturbed, simple_system, snapshot_of_slabs  # noqa: F401  (the fixture)
from ephemeris_explorer_amd.systems import load_ship, soi_parents, soi_radii
from oracle import orc
from test_gpu_craft_plot import RES, views_for

pytestmark = pytest.mark.gpu

SEED = 20261018          # test_gpu_craft_segments.py's: copies 4 and 5 miss the capture and fly by Mars


def config(start, end, **more):
    return {"start": start, "end": end, "tan2_angular_resolution": RES, "max_points_per_segment": 4000, **more}


def check(batch, requests, crafts, burns, osol, what, with_events=True, inputs=None):
    """one call against the restatement: every record, and out_first -> (markers, first)"""
    listed = np.arange(len(requests)) if crafts is None else np.asarray(crafts, dtype=np.int64)
    events, knots = inputs or R.inputs_of(batch, with_events)
    want, want_first = R.expected_markers(requests, listed, events, knots, burns, osol)
    markers, first = batch.plot_markers(requests, craft=crafts)
    got = R.record_tuples(markers)
    assert R.same_markers(got, want), (what, len(got), len(want), R.first_difference(got, want))
    assert np.array_equal(first, want_first), what
    assert np.array_equal(np.searchsorted(markers["request"], np.arange(len(requests) + 1)), first), what
    return markers, first


@pytest.fixture(scope="module")
def wave_case(gpu, simple_system):
    """7 craft to start + 215 d with events on: the six of test_gpu_craft_segments.py's wave_case (the ship, the ship without its
    last burn, four perturbed copies with all four burns) and the ship with its first burn given in the inertial frame"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    pos, vel = perturbed(ship, 6, SEED)
    pos[1], vel[1] = ship.pos, ship.vel
    pos, vel = np.vstack([pos, ship.pos]), np.vstack([vel, ship.vel])
    full = ship.burn_tuples(s.names)
    inertial = [(full[0][0], full[0][1], full[0][2], -1)] + full[1:]
    burns = [full, full[:-1]] + [full] * 4 + [inertial]
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), burns,
                                max_knots=8192).enable_events(soi_radii(s), 16, 8192)
    batch.propagate(ship.start + 215 * DAY)
    assert (batch.status()["status"] == 0).all() and (batch.event_counts()[2] == 0).all()
    return dict(batch=batch, burns=burns, parents=soi_parents(s), ship=ship, pos=pos, vel=vel, inputs=R.inputs_of(batch))


def frame_of(gpu, batch, view, parents, t0):
    """the frame's plots and their marker requests: one whole-window config per craft -> (segments, requests, crafts)"""
    segments, plots = batch.plot_segments(view, [config(t0, t0 + 400 * DAY)] * batch.n, parents)
    return segments, gpu.marker_requests(segments, plots), segments["plot"].astype(np.int64)


def test_wave_form(gpu, simple_system, wave_case):
    """1. the markers of every plot of the frame under both views; every kinds mask on one craft; craft == NULL; a shuffled craft list
    with repeats; the positions against eph_craft_batch_eval"""
    s, sol, eph, osol = simple_system
    batch, burns, parents, ship, inputs = (wave_case[k] for k in ("batch", "burns", "parents", "ship", "inputs"))
    t0 = ship.start
    checked = 0
    for v, view in enumerate(views_for(s.epoch)):
        segments, requests, crafts = frame_of(gpu, batch, view, parents, t0)
        markers, first = check(batch, requests, crafts, burns, osol, f"view {v}", inputs=inputs)
        checked += len(markers)
        # what the case must contain, so that an empty comparison cannot pass
        assert set(int(k) for k in markers["kind"]) == {0, 1, 2, 3, 4, 5}
        lo = np.array([requests[int(r)]["first"] for r in markers["request"]])
        hi = np.array([requests[int(r)]["last"] for r in markers["request"]])
        assert (markers["time"] == lo).any() and (markers["time"] == hi).any() and ((markers["time"] > lo) & (markers["time"] < hi)).any()
        identity = markers[(markers["kind"] == 0) & (markers["body"] == -1)]
        assert len(identity) and all(tuple(m["frame"]) == R.IDENTITY and m["status"] == 3 for m in identity)
        relative = markers[(markers["kind"] == 0) & (markers["body"] >= 0)]
        assert len(relative) >= 6 * 3 and (relative["status"] == 3).all() and all(tuple(m["frame"]) != R.IDENTITY for m in relative)
        over = np.flatnonzero(segments["overlapping"] == 1)
        assert len(over) and all(requests[int(i)]["kinds"] & 2 == 0 for i in over if requests[int(i)]["kinds"])
        assert any(requests[int(i)]["kinds"] for i in over)
        assert not (markers["kind"][np.isin(markers["request"], over)] == 1).any()
        assert (markers["status"] & 1).all()                          # the table and the knots cover every epoch here
        assert (markers["apsis_distance"][np.isin(markers["kind"], (2, 3))] > 0.0).all()
        names = [gpu.marker_name(s.names, m) for m in markers[first[0]:first[1]]]
        assert names[0] == "Earth Transition" and "Earth Apoapsis" in names and names[-1] == "Start"
        # the positions through an independent device path: eph_craft_batch_eval, every craft its own epochs, per reference body
        reference = np.array([requests[int(r)]["reference_body"] for r in markers["request"]])
        craft_of = crafts[markers["request"]]
        for body in sorted(set(int(b) for b in reference)):
            rows = [np.flatnonzero((reference == body) & (craft_of == c)) for c in range(batch.n)]
            at = np.full((max(len(r) for r in rows), batch.n), t0)
            for c, r in enumerate(rows):
                at[:len(r), c] = markers["time"][r]
            pos, _, inside = batch.eval(at, reference_body=body)
            for c, r in enumerate(rows):
                assert inside[:len(r), c].all() and np.array_equal(bits(pos[:len(r), c]), bits(markers["position"][r])), (v, body, c)
    assert checked >= 2 * 7 * 10                                        # (per craft at least 3 burns, 3 transitions, 2 apsides, 2 bounds)
    view = views_for(s.epoch)[0]
    segments, requests, crafts = frame_of(gpu, batch, view, parents, t0)
    # every mask on the plots of craft 1 (the flyby: an overlapping copy among them)
    mine = [q for q, c in zip(requests, crafts) if c == 1]
    masked = [{**q, "kinds": k} for k in range(16) for q in mine]
    markers, first = check(batch, masked, [1] * len(masked), burns, osol, "masks", inputs=inputs)
    per_mask = np.add.reduceat(np.diff(first), np.arange(0, len(masked), len(mine)))
    assert per_mask[0] == 0 and per_mask[15] == per_mask[1] + per_mask[2] + per_mask[4] + per_mask[8] and (per_mask[[1, 2, 4, 8]] > 0).all()
    # craft == NULL: request r is craft r; one dict for all
    whole = {"reference_body": s.names.index("Sun"), "kinds": 15, "first": t0, "last": t0 + 400 * DAY}
    markers, first = check(batch, [whole] * batch.n, None, burns, osol, "craft == NULL", inputs=inputs)
    again, _ = batch.plot_markers(whole)
    assert again.tobytes() == markers.tobytes() and (np.diff(first) >= 8).all() and np.diff(first).max() > 90
    # a shuffled craft list with repeats
    rng = np.random.default_rng(3)
    pick = np.concatenate([rng.permutation(len(requests)), rng.integers(0, len(requests), 20), [5, 5, 5]])
    check(batch, [requests[i] for i in pick], crafts[pick], burns, osol, "shuffled", inputs=inputs)


def test_statuses(gpu):
    """2. on a table of its own: after eph_ephemeris_clear(Earth, before = start + 1 d) the markers of the Earth-relative plots before
    that epoch lose bit 0 and the burn in Earth's frame loses bit 1, plots relative to the Sun are unaffected; on a clone, after
    reset_knots and a further propagate, events before the drained slab's span lose bit 0; reset_events leaves one transition and
    no apsides; a batch without events gives manoeuvres and bounds only"""
    s = load_system("simple_solar_system_2433282.5")
    ship = load_ship(SHIP)
    g = gpu.NBodyPropagator.from_system(s)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    pieces = []
    for t in (s.epoch + 8 * DAY, s.epoch + 16 * DAY):
        g.step_to(t)
        assert o.step_to(t) == 0
        pieces.append((g.take_solution(), o.take_solution()))
    eph, olive = gpu.Ephemeris(pieces[0][0], s.mu), pieces[0][1].clone()
    eph.append(pieces[1][0])
    assert olive.append(pieces[1][1])
    sun, earth = s.names.index("Sun"), s.names.index("Earth")
    n, t0 = 3, ship.start
    pos, vel = perturbed(ship, n, 81)
    full = ship.burn_tuples(s.names)
    assert full[0][3] == earth and full[1][3] == sun
    burns = [full] * n
    make = lambda: gpu.SpacecraftBatch(eph, t0, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), burns,   # noqa: E731
                                       max_knots=4096)
    batch = make().enable_events(soi_radii(s), 16, 256)
    batch.propagate(t0 + 8 * DAY)
    assert (batch.status()["status"] == 0).all() and (batch.event_counts()[2] == 0).all()
    inputs = R.inputs_of(batch)
    parents, view = soi_parents(s), views_for(s.epoch)[1]
    cfgs = [config(t0, t0 + 400 * DAY, reference_body=body) for body in (-1, sun, earth) for _ in range(n)]
    crafts = np.tile(np.arange(n), 3)
    segments, plots = batch.plot_segments(view, cfgs, parents, craft=crafts)
    requests, listed = gpu.marker_requests(segments, plots), crafts[segments["plot"]]
    before, _ = check(batch, requests, listed, burns, olive, "the whole table", inputs=inputs)
    assert (before["status"] & 1).all() and (before["status"][before["kind"] == 0] == 3).all()
    clone = batch.clone()
    # Earth's spline cleared before start + 1 d: UniformSpline::clear_before drops the polynomial that holds the epoch too
    eph.clear_before(t0 + DAY, body=earth)
    olive.clear_before(t0 + DAY, body=earth)
    earth_start = olive.info(earth)[0]
    assert t0 + DAY < earth_start < t0 + 8 * DAY and eph.info(earth) == olive.info(earth) and eph.info(sun)[0] == s.epoch
    after, _ = check(batch, requests, listed, burns, olive, "Earth cleared", inputs=inputs)
    reference = np.array([requests[int(r)]["reference_body"] for r in after["request"]])
    early = after["time"] < earth_start
    gone = (reference == earth) & early
    assert gone.any() and ((reference == earth) & ~early).any() and (after["status"][gone] & 1 == 0).all() and (after["status"][~gone] & 1 == 1).all()
    assert (bits(after["position"][gone]) == 0).all() and (bits(after["distance"][gone]) == 0).all()      # +0.0
    in_earths_frame = (after["kind"] == 0) & (after["body"] == earth)
    assert in_earths_frame.any() and (after["status"][in_earths_frame] & 2 == 0).all() and (bits(after["frame"][in_earths_frame]) == 0).all()
    in_suns_frame = (after["kind"] == 0) & (after["body"] == sun)
    assert in_suns_frame.any() and (after["status"][in_suns_frame] & 2 == 2).all()
    assert ((reference == earth) & in_suns_frame & (after["status"] == 2)).any()        # the frame without the position
    suns = reference == sun                                           # relative to the Sun: only the frames built on Earth change
    assert suns.any() and after[suns & ~in_earths_frame].tobytes() == before[suns & ~in_earths_frame].tobytes()
    assert (suns & in_earths_frame).any() and (after["status"][suns & in_earths_frame] == 1).all()
    assert after["position"][suns].tobytes() == before["position"][suns].tobytes()
    assert after["distance"][suns].tobytes() == before["distance"][suns].tobytes()
    assert after[~early].tobytes() == before[~early].tobytes()
    # a drained slab: events before its span have no position, burns no frame; Start is the drained knot
    clone.reset_knots()
    clone.propagate(t0 + 9 * DAY)
    assert (clone.status()["status"] == 0).all()
    wide = {"reference_body": -1, "kinds": 15, "first": t0, "last": t0 + 400 * DAY}
    drained, first = check(clone, [wide] * n, None, burns, olive, "drained slab")
    knot0 = np.array([clone.knots(c)[0][0] for c in range(n)])
    knot1 = np.array([clone.knots(c)[0][-1] for c in range(n)])
    old = drained["time"] < knot0[drained["request"]]
    held = ~old & (drained["time"] <= knot1[drained["request"]])
    assert old.any() and held.any() and (drained["status"][~held] == 0).all() and (drained["status"][held] & 1 == 1).all()
    assert (drained["kind"][old] == 0).any() and (drained["kind"][old] == 1).any() and (drained["kind"][old] >= 2).any()
    assert all(drained[first[c + 1] - 2]["kind"] == 4 and drained[first[c + 1] - 2]["time"] == knot0[c] for c in range(n))
    # reset_events: one transition, no apsides
    clone.reset_events()
    reset, _ = check(clone, [wide] * n, None, burns, olive, "after reset_events")
    assert [int((reset["kind"] == k).sum()) for k in range(6)] == [4 * n, n, 0, 0, n, n]
    # without events: manoeuvres and bounds only
    plain = make()
    plain.propagate(t0 + 8 * DAY)
    bare, _ = check(plain, [wide] * n, None, burns, olive, "no events", with_events=False)
    assert [int((bare["kind"] == k).sum()) for k in range(6)] == [4 * n, 0, 0, 0, n, n]


_DEALT_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import ephemeris_explorer_amd as ea
import craft_markers_restatement as R
from craft_cases import DAY, SHIP, perturbed
from test_gpu_craft_plot import RES, views_for
from ephemeris_explorer_amd.systems import load_system, load_ship, parse_epoch, soi_parents, soi_radii
from oracle import orc
s = load_system(sys.argv[1] + "/tests/golden/systems/simple_solar_system_2433282.5")
ship = load_ship(SHIP)
end = parse_epoch("1951-01-01 00:00:00")
eph = ea.Ephemeris(ea.NBodyPropagator.from_system(s).propagate(end), s.mu)
o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
assert o.step_to(end) == 0
osol = o.take_solution()
assert all(eph.info(b) == osol.info(b) for b in range(s.n))
n = 192
pos, vel = perturbed(ship, n, 20261018)
full = ship.burn_tuples(s.names)
burns = [(full, full[:-1], full[:1])[c % 3] for c in range(n)]
batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, ea.AdaptiveParams.default(ship.tolerance), burns,
                           max_knots=8192).enable_events(soi_radii(s), 16, 8192)
batch.propagate(ship.start + 215 * DAY)
st = batch.status()["status"]
assert np.isin(st, (0, ea.KNOTS_FULL)).all() and (st == 0).sum() >= n // 3, st
cfg = {"start": ship.start, "end": ship.start + 400 * DAY, "tan2_angular_resolution": RES, "max_points_per_segment": 512}
segments, plots = batch.plot_segments(views_for(s.epoch)[0], cfg, soi_parents(s))
requests, crafts = ea.marker_requests(segments, plots), segments["plot"].astype(np.int64)
events, knots = R.inputs_of(batch)
rng = np.random.default_rng(5)
pick = np.concatenate([rng.permutation(len(requests)), rng.integers(0, len(requests), 40), [7, 7, 7]])
whole = {"reference_body": s.names.index("Earth"), "kinds": 15, "first": ship.start, "last": ship.start + 400 * DAY}
kinds, total, per_craft = set(), 0, None
for what, rq, cr in (("craft == NULL", [whole] * n, None), ("the frame", requests, crafts),
                     ("shuffled", [requests[i] for i in pick], crafts[pick])):
    listed = np.arange(n) if cr is None else cr
    want, want_first = R.expected_markers(rq, listed, events, knots, burns, osol)
    markers, first = batch.plot_markers(rq, craft=cr)
    got = R.record_tuples(markers)
    assert R.same_markers(got, want), (what, len(got), len(want), R.first_difference(got, want))
    assert np.array_equal(first, want_first), what
    kinds |= set(int(k) for k in markers["kind"])
    total += len(markers)
    if cr is None:
        per_craft = np.diff(first)
assert kinds == {0, 1, 2, 3, 4, 5}, kinds
# the balance case: the craft that stay in Earth orbit carry many times the apsides of the neighbours that fly by Mars
print("markers per craft:", int(per_craft[2::3].min()), int(per_craft.max()), int(np.median(per_craft[0::3])), int(np.median(per_craft[1::3])))
assert per_craft[2::3].min() > 4 * np.median(per_craft[1::3]), (per_craft[2::3].min(), np.median(per_craft[1::3]))
print("dealt lanes ok", total)
'''


def test_dealt_lanes(gpu):
    """3. the thread form (forced in a child process: the form is read once per process): 192 craft whose burn lists differ from craft
    to craft, dealt to the lanes -- every third stays in Earth orbit and carries far more apsides than its neighbours; craft == NULL,
    the frame's requests and a shuffled list with repeats, every record against the restatement"""
    env = dict(os.environ, EPH_CRAFT_FORM="thread")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _DEALT_SCRIPT, str(ROOT)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0 and "dealt lanes ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


def test_the_batch_is_untouched(gpu, simple_system, wave_case):
    """4. summary, knot slabs and events are bit-equal before and after; a following propagate equals a twin's that never asked; a
    clone gives the same bytes"""
    s, sol, eph, osol = simple_system
    batch, parents, ship = (wave_case[k] for k in ("batch", "parents", "ship"))
    a, twin = batch.clone(), batch.clone()
    before = snapshot_of_slabs(a)
    segments, requests, crafts = frame_of(gpu, a, views_for(s.epoch)[1], parents, ship.start)
    markers, first = a.plot_markers(requests, craft=crafts)
    assert len(markers) >= 7 * 10
    assert snapshot_of_slabs(a) == before == snapshot_of_slabs(twin)
    same, same_first = twin.plot_markers(requests, craft=crafts)
    assert same.tobytes() == markers.tobytes() and np.array_equal(first, same_first)
    a.propagate(ship.start + 217 * DAY)
    twin2 = batch.clone()
    twin2.propagate(ship.start + 217 * DAY)
    assert snapshot_of_slabs(a) == snapshot_of_slabs(twin2)


def test_sizing_and_refusals(gpu, simple_system, wave_case):
    """5. the sizing call, a record array one short, every refusal: poisoned buffers stay poisoned"""
    s, sol, eph, osol = simple_system
    batch, ship = (wave_case[k] for k in ("batch", "ship"))
    L, h = batch._L, batch._h
    i64p = C.POINTER(C.c_int64)
    n, t0 = batch.n, ship.start
    expected, expected_first = batch.plot_markers({"reference_body": -1, "kinds": 15, "first": t0, "last": t0 + 400 * DAY})
    total = len(expected)
    assert total >= n * 10 and expected_first[n] == total
    rows = total + 2
    marks = np.full(rows * 144, 0xA5, np.uint8)
    first = np.full(n + 1, -99, np.int64)

    def poisoned(but_first=False):
        return (marks == 0xA5).all() and (but_first or (first == -99).all())

    def one(ref=-1, kinds=15, lo=t0, hi=t0 + 400 * DAY):
        return gpu.MarkerRequest(ref, kinds, lo, hi)

    def call(rqs, n_requests=None, craft=None, cap=rows, records=True, fst=True, handle=h):
        arr = (gpu.MarkerRequest * max(len(rqs), 1))(*rqs) if rqs is not None else None
        cr = None if craft is None else np.asarray(craft, dtype=np.int64)
        return L.eph_craft_batch_plot_markers(handle, len(rqs) if n_requests is None else n_requests, arr,
                                              None if cr is None else cr.ctypes.data_as(i64p), cap,
                                              marks.ctypes.data_as(C.POINTER(gpu.PlotMarker)) if records else None,
                                              first.ctypes.data_as(i64p) if fst else None)
    bad = gpu.ERR_BAD_ARGUMENT
    ok = [one()] * n
    assert call(ok, handle=None) == bad
    assert call(ok, n_requests=-1) == bad and call(None, n_requests=1) == bad and call(ok, fst=False) == bad
    assert call(ok[:1], craft=[n]) == bad and call(ok[:1], craft=[-1]) == bad and call(ok[:2], craft=[0, n]) == bad
    assert call(ok + ok[:1]) == bad                                     # craft == NULL: at most one request per craft
    assert call([one(ref=-2)]) == bad and call([one(ref=s.n)]) == bad and call([one(), one(ref=s.n)]) == bad
    assert call([one(kinds=-1)]) == bad and call([one(kinds=16)]) == bad
    assert call([one(lo=float("nan"))]) == bad and call([one(hi=float("nan"))]) == bad
    assert call(ok, cap=-1) == bad and call(ok, records=False) == bad
    assert call([], n_requests=0) == 0 and call(None, n_requests=0, cap=0, records=False, fst=False) == 0
    assert poisoned()
    # one record short: the needed total comes back in out_first, nothing else is written
    assert call(ok, cap=total - 1) == bad
    assert list(first) == list(expected_first) and poisoned(but_first=True)
    first[:] = -99
    assert call(ok, cap=0, records=False) == bad and list(first) == list(expected_first) and poisoned(but_first=True)   # the sizing call
    # a call with nothing to return needs no array
    first[:] = -99
    assert call([one(kinds=0)] * n, cap=0, records=False) == 0 and (first == 0).all() and poisoned(but_first=True)
    # the filling call: the records, and nothing beyond them
    assert call(ok) == 0
    assert marks[:total * 144].tobytes() == expected.tobytes() and (marks[total * 144:] == 0xA5).all()
    # first > last: valid, and empty
    assert call([one(lo=t0 + DAY, hi=t0)] * n) == 0 and (first == 0).all()
