"""-m gpu: eph_craft_batch_plot_points -- the adaptive plot sampler on the knot slabs of a spacecraft batch -- against the Python
restatement of compute_plot_points_parallel / PlotPoints::new (oracle_plot of craft_cases.py, evaluations by the C oracle) on the
knots batch.knots(c) returns, and against eph_plot_points fed with those knots. Every comparison is on bit patterns (u64 epochs,
u32 points); there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_system
from craft_cases import DAY, SHIP, gathered_knots, oracle_plot, perturbed, simple_system, snapshot_of_slabs  # noqa: F401  (the fixture)
from ephemeris_explorer_amd.systems import load_ship, parse_epoch
from oracle import orc

pytestmark = pytest.mark.gpu

RES = float(np.float32(1.0) * np.float32(0.000290888) * np.float32(0.7853982))          # threshold * ARC_MINUTE * fov
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
N_DRAWING = 5                                                                           # the first five requests of requests_for()
CAPPED = 4


def views_for(t0):
    return [{"camera_position": (1.2e8, -3.0e8, 2.0e8), "current": t0 + 30 * DAY},
            {"camera_position": (5.0e5, 2.0e5, -3.0e5), "current": t0 + 3 * DAY, "grid_matrix3": ROT,
             "grid_translation": (10.0, -20.0, 5.0), "cell_offset": (1.0e6, 2.0e6, -5.0e5)}]


def requests_for(s):
    """per craft: five drawing requests (references none / Sun / Earth / Mars, the capped one), then bound 1 and 2, a disabled plot,
    start > end, max_points 0"""
    t0 = s.epoch
    sun, earth, mars = (s.names.index(x) for x in ("Sun", "Earth", "Mars"))
    w = {"start": t0, "end": t0 + 400 * DAY}
    return [
        {**w, "reference_body": -1, "tan2_angular_resolution": RES, "max_points": 4000},
        {**w, "reference_body": sun, "tan2_angular_resolution": RES, "max_points": 4000},
        {**w, "reference_body": earth, "tan2_angular_resolution": RES * 4, "max_points": 4000},
        {**w, "reference_body": mars, "tan2_angular_resolution": RES, "max_points": 4000},
        {**w, "reference_body": -1, "tan2_angular_resolution": RES * 0.25, "max_points": 64},        # the cap cuts it
        {**w, "reference_body": sun, "bound": 1, "tan2_angular_resolution": RES, "max_points": 4000},
        {**w, "reference_body": earth, "bound": 2, "tan2_angular_resolution": RES, "max_points": 4000},
        {**w, "reference_body": mars, "enabled": 0, "tan2_angular_resolution": RES, "max_points": 100},
        {"start": t0 + 50 * DAY, "end": t0 + 40 * DAY, "reference_body": -1, "tan2_angular_resolution": RES, "max_points": 100},
        {**w, "reference_body": sun, "tan2_angular_resolution": RES, "max_points": 0},
    ]


def same_plot(a, b):
    return (a[0] == b[0] and np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64) and len(a[2]) == len(b[2]) and
            np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)))


def assert_same_plots(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_plot(g, w), f"{what}: plot {i} differs (status {g[0]} / {w[0]}, {len(g[2])} / {len(w[2])} points)"


def restated(s, osol, knots, view, rq):
    """the restatement's answer in plot_points()'s form: (status, failed_at, t, xyz)"""
    kind, want = oracle_plot(s, osol, knots, view, {**rq, "knots": (0, len(knots[0]))})
    assert kind == "ok", kind
    return (0, 0.0, np.array([w[0] for w in want], dtype=np.float64),
            np.array([w[1] for w in want], dtype=np.float32).reshape(-1, 3))


def by_plot_points(gpu, eph, batch, crafts, view, requests):
    """eph_plot_points (unchanged, itself pinned to the restatement) fed with the knots read back from the batch: one call per craft"""
    out = []
    nk = batch.status()["nknots"]
    for c, rq in zip(crafts, requests):
        knots = batch.knots(int(c), nk[int(c)])
        out += gpu.plot_points(eph, view, [{**rq, "knots": (0, len(knots[0]))}], knots)
    return out


@pytest.fixture(scope="module")
def thread_case(gpu, simple_system):
    """the thread form with dealt lanes: 16 384 perturbed copies over the first 220 days (all four burns), max_knots = 4096"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 16384
    pos, vel = perturbed(ship, n, 20261017)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance),
                                [ship.burn_tuples(s.names)] * n, max_knots=4096)
    batch.propagate(ship.start + 220 * DAY)
    st = batch.status()
    assert np.isin(st["status"], (0, gpu.KNOTS_FULL)).all() and st["status"][0] == 0
    return dict(batch=batch, n=n, nknots=st["nknots"])


def test_wave_form_every_plot_against_the_restatement(gpu, simple_system):
    """1. 192 craft to 1951-01-01 (one wave per craft): every request of every craft in both views against the restatement"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 192
    assert ship.start == s.epoch
    pos, vel = perturbed(ship, n, 20261016)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance),
                                [ship.burn_tuples(s.names)] * n, max_knots=20000)
    batch.propagate(parse_epoch("1951-01-01 00:00:00"))
    st = batch.status()
    assert (st["status"] == 0).all()
    requests = requests_for(s)
    knots = [batch.knots(c, st["nknots"][c]) for c in range(n)]
    assert len(knots[0][0]) > 10000                                                     # the app's ship: ~13 000 knots
    done = cut = 0
    for view in views_for(s.epoch):
        for r, rq in enumerate(requests):
            got = batch.plot_points(view, rq)                                           # one dict for all craft, craft == NULL
            assert len(got) == n
            for c in range(n):
                want = restated(s, osol, knots[c], view, rq)
                assert same_plot(got[c], want), (r, c, got[c][0], len(got[c][2]), len(want[2]))
                if r < N_DRAWING or r in (5, 6):
                    assert got[c][0] == 0 and len(got[c][2]) >= 2, (r, c)
                else:
                    assert got[c][0] == 0 and len(got[c][2]) == 0, (r, c)
                if r == CAPPED:                                                         # exactly 64 wherever the cap cuts
                    uncut = len(restated(s, osol, knots[c], view, {**rq, "max_points": 4000})[2])
                    assert len(got[c][2]) == min(uncut, 64), (r, c, len(got[c][2]), uncut)
                    cut += uncut > 64
                done += 1
    assert done == 2 * len(requests) * n                                                # no plot is left out
    assert cut > 0                                                                      # the cap does cut


def test_thread_form_dealt_lanes(gpu, simple_system, thread_case):
    """2. 16 384 craft dealt to the lanes: all plots against eph_plot_points on the knots read back, every 64th craft against the
    restatement; craft == NULL and a shuffled craft list with repeats give the same rows per craft"""
    s, sol, eph, osol = simple_system
    batch, n, nknots = thread_case["batch"], thread_case["n"], thread_case["nknots"]
    assert n > 12288
    requests = requests_for(s)
    views = views_for(s.epoch)
    knots, first, count = gathered_knots(batch, nknots)
    sample = {c: batch.knots(c, nknots[c]) for c in range(0, n, 64)}                    # 256 of them, none skipped
    assert len(sample) == 256
    for c, k in sample.items():                                                         # the gather itself
        assert all(np.array_equal(a, b[first[c]:first[c] + count[c]]) for a, b in zip(k, knots))
    rng = np.random.default_rng(5)
    checked = 0
    for v, view in enumerate(views):
        for r, rq in enumerate(requests):
            got = batch.plot_points(view, rq)
            assert len(got) == n
            want = gpu.plot_points(eph, view, [{**rq, "knots": (int(first[c]), int(count[c]))} for c in range(n)], knots)
            assert_same_plots(got, want, f"view {v} request {r}")
            for c, k in sample.items():
                assert same_plot(got[c], restated(s, osol, k, view, rq)), (v, r, c, got[c][0], len(got[c][2]))
                checked += 1
            if r < N_DRAWING:
                assert all(g[0] == 0 and len(g[2]) >= 2 for g in got)
            if r == CAPPED:                                                             # exactly 64 wherever the cap cuts
                uncut = batch.plot_points(view, {**rq, "max_points": 4000})
                for c, k in sample.items():
                    assert same_plot(uncut[c], restated(s, osol, k, view, {**rq, "max_points": 4000})), (v, c)
                assert all(len(g[2]) == min(len(u[2]), 64) for g, u in zip(got, uncut)) and any(len(u[2]) > 64 for u in uncut)
            if v == 0 and r in (1, CAPPED):
                crafts = np.concatenate([rng.permutation(n), rng.integers(0, n, 1000), [7, 7, 7]])    # shuffled, with repeats
                listed = batch.plot_points(view, rq, craft=crafts)
                assert_same_plots(listed, [got[c] for c in crafts], "craft list")
    assert checked == 2 * len(requests) * 256
    # different requests per plot of the same craft
    crafts = np.repeat(np.array([0, 9000, 16383]), len(requests))
    mixed = batch.plot_points(views[1], requests * 3, craft=crafts)
    assert_same_plots(mixed, by_plot_points(gpu, eph, batch, crafts, views[1], requests * 3), "one craft, several requests")


def test_more_than_one_pass(gpu, simple_system, thread_case):
    """3. 16 384 craft x 2 references at capacity 512: 335 MB of results, more than one staging pass; equal, plot for plot, to the same
    requests issued in chunks that fit one pass"""
    s, sol, eph, osol = simple_system
    batch, n = thread_case["batch"], thread_case["n"]
    sun, earth = s.names.index("Sun"), s.names.index("Earth")
    base = {"start": s.epoch, "end": s.epoch + 400 * DAY, "tan2_angular_resolution": RES, "max_points": 512}
    requests = [{**base, "reference_body": sun}] * n + [{**base, "reference_body": earth}] * n
    crafts = np.concatenate([np.arange(n), np.arange(n)])
    assert 2 * n * (512 * 20 + 20) > 256 << 20
    view = views_for(s.epoch)[0]
    whole = batch.plot_points(view, requests, craft=crafts)
    assert all(g[0] == 0 and len(g[2]) >= 2 for g in whole)
    chunk = 4096
    assert chunk * (512 * 20 + 20) < 256 << 20
    parts = []
    for i in range(0, 2 * n, chunk):
        parts += batch.plot_points(view, requests[i:i + chunk], craft=crafts[i:i + chunk])
    assert_same_plots(whole, parts, "multi-pass")


def test_the_batch_is_untouched(gpu, simple_system):
    """4. summary, knot slabs, events and a following propagate are bit-equal with and without a plot call in between; a clone plots the
    same; after reset_knots and after a restart of a subset the plot is eph_plot_points on the new knots; one knot draws nothing"""
    from ephemeris_explorer_amd.systems import soi_radii
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 40
    pos, vel = perturbed(ship, n, 11)
    burns = ship.burn_tuples(s.names)
    requests = requests_for(s)
    view = views_for(s.epoch)[1]
    mid, end = ship.start + 60 * DAY, ship.start + 80 * DAY
    a, b = (gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), [burns] * n,
                                max_knots=20000).enable_events(soi_radii(s)) for _ in range(2))
    fresh = a.plot_points(view, requests[0])                                            # one knot: nothing drawn
    assert all(g[0] == 0 and len(g[2]) == 0 for g in fresh)
    a.propagate(mid)
    b.propagate(mid)
    before = snapshot_of_slabs(a)
    crafts = np.repeat(np.arange(n), len(requests))
    got = a.plot_points(view, requests * n, craft=crafts)
    assert snapshot_of_slabs(a) == before == snapshot_of_slabs(b)
    assert_same_plots(got, by_plot_points(gpu, eph, a, crafts, view, requests * n), "before")
    assert_same_plots(a.clone().plot_points(view, requests * n, craft=crafts), got, "clone")
    a.propagate(end)
    b.propagate(end)
    assert snapshot_of_slabs(a) == snapshot_of_slabs(b)
    # a restart of a subset: the selected craft's plots follow their new knots
    news = [list(burns) for _ in range(n)]
    sel = np.arange(n) % 3 == 0
    for c in np.flatnonzero(sel):
        st_, en, acc, ref = burns[2]
        news[c][2] = (st_, en, np.asarray(acc) * 1.01, ref)
    epoch, outcome = a.restart(news, which=sel)
    assert (outcome[sel] == 0).all()
    a.propagate(end)
    drawn = a.plot_points(view, requests[3])
    assert_same_plots(drawn, by_plot_points(gpu, eph, a, np.arange(n), view, [requests[3]] * n), "after restart")
    kept = b.plot_points(view, requests[3])
    assert all(same_plot(drawn[c], kept[c]) for c in np.flatnonzero(~sel)) and not all(same_plot(drawn[c], kept[c]) for c in np.flatnonzero(sel))
    # a drained slab: only its span is drawn
    last = np.array([b.knots(c)[0][-1] for c in range(n)])
    b.reset_knots()
    assert all(g[0] == 0 and len(g[2]) == 0 for g in b.plot_points(view, requests[0]))  # one knot again
    b.propagate(end + 60 * DAY)                                                         # (a cruise step can be days long)
    drained = b.plot_points(view, requests[1])
    assert_same_plots(drained, by_plot_points(gpu, eph, b, np.arange(n), view, [requests[1]] * n), "drained slab")
    stb = b.status()
    assert (stb["status"] == 0).all() and (stb["nknots"] >= 2).all(), (stb["status"], stb["nknots"], b.event_counts()[2])
    assert [len(g[2]) >= 2 for g in drained] == [True] * n, [len(g[2]) for g in drained]
    assert [g[2][0] for g in drained] == list(last), ([g[2][0] for g in drained], list(last))
    want = restated(s, osol, b.knots(0), view, requests[1])
    assert same_plot(drained[0], want)


def test_live_table(gpu):
    """5. a relative plot whose window runs past the table's end stops at the reference's end; after eph_ephemeris_append the same call
    reaches further; both equal the restatement on the respective table"""
    s = load_system("simple_solar_system_2433282.5")
    ship = load_ship(SHIP)
    g = gpu.NBodyPropagator.from_system(s)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    pieces = []
    for t in (s.epoch + 100 * DAY, s.epoch + 200 * DAY):
        g.step_to(t)
        assert o.step_to(t) == 0
        pieces.append((g.take_solution(), o.take_solution()))
    eph, olive = gpu.Ephemeris(pieces[0][0], s.mu), pieces[0][1].clone()
    eph.append(pieces[1][0])
    assert olive.append(pieces[1][1])
    n = 6
    pos, vel = perturbed(ship, n, 81)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance),
                                [ship.burn_tuples(s.names)] * n, max_knots=20000)
    batch.propagate(s.epoch + 150 * DAY)
    assert (batch.status()["status"] == 0).all()
    earth = s.names.index("Earth")
    view = views_for(s.epoch)[0]
    rq = {"start": s.epoch, "end": s.epoch + 400 * DAY, "reference_body": earth, "tan2_angular_resolution": RES, "max_points": 4000}
    knots = [batch.knots(c) for c in range(n)]
    long_ = batch.plot_points(view, rq)
    # the table shrinks under the batch (the knots stay): the reference ends before the craft do
    cut = max(pieces[1][1].info(b)[0] for b in range(s.n))                              # where the second piece starts (per body: <= cut)
    eph.clear_after(cut)
    olive.clear_after(cut)
    assert all(eph.info(b) == olive.info(b) == pieces[0][1].info(b) for b in range(s.n))
    ref_end = olive.info(earth)[0] + olive.info(earth)[1] * float(olive.info(earth)[2])
    assert s.epoch + 100 * DAY <= ref_end < min(k[0][-1] for k in knots)
    short = batch.plot_points(view, rq)
    for c in range(n):
        assert same_plot(short[c], restated(s, olive, knots[c], view, rq)), c
        assert short[c][0] == 0 and short[c][2][-1] == ref_end                          # stops at the reference's end
    inertial = batch.plot_points(view, {**rq, "reference_body": -1})                    # no reference: the whole craft span
    assert all(g[2][-1] == knots[c][0][-1] for c, g in enumerate(inertial))
    eph.append(pieces[1][0])
    assert olive.append(pieces[1][1])
    again = batch.plot_points(view, rq)
    for c in range(n):
        assert same_plot(again[c], restated(s, olive, knots[c], view, rq)), c
        assert again[c][2][-1] == knots[c][0][-1] and len(again[c][2]) > len(short[c][2])
    assert_same_plots(again, long_, "the table as it was")


def test_failure_statuses_and_refusals(gpu, simple_system):
    """6. the degenerate view of test_plot_points_argument_errors: EPH_MAX_ITERATIONS_REACHED with count 1; every refusal returns
    EPH_ERR_BAD_ARGUMENT and leaves poisoned outputs poisoned"""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 4
    pos, vel = perturbed(ship, n, 12)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=256)
    batch.propagate(ship.start + 3600.0)
    L, h = batch._L, batch._h
    dp, fp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    v = gpu.PlotView()
    v.camera_position[:] = [1.0e8, 2.0e8, 3.0e8]
    v.grid_matrix3[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    v.current = s.epoch
    cap = 10
    ot, ox = np.full(n * cap, -7.25), np.full(n * cap * 3, -7.25, dtype=np.float32)
    cnt, stt, fail = np.full(n, -99, np.int64), np.full(n, -99, np.int32), np.full(n, -7.25)
    outs = [ot.ctypes.data_as(dp), ox.ctypes.data_as(fp), cnt.ctypes.data_as(i64p), stt.ctypes.data_as(i32p), fail.ctypes.data_as(dp)]

    def poisoned():
        return (ot == -7.25).all() and (ox == np.float32(-7.25)).all() and (cnt == -99).all() and (stt == -99).all() and (fail == -7.25).all()

    def request(source=-1, ref=-1, first=0, count=0, bound=0, max_points=cap):
        return gpu.PlotRequest(source, ref, first, count, s.epoch, s.epoch + 3600.0, bound, 1, 1e-4, max_points)

    def call(rqs, n_plots=None, craft=None, capacity=cap, view=v, o=outs, handle=h):
        arr = (gpu.PlotRequest * max(len(rqs), 1))(*rqs) if rqs is not None else None
        cr = None if craft is None else np.asarray(craft, dtype=np.int64)
        return L.eph_craft_batch_plot_points(handle, None if view is None else C.byref(view), len(rqs) if n_plots is None else n_plots, arr,
                                             None if cr is None else cr.ctypes.data_as(i64p), capacity, *o)
    bad = gpu.ERR_BAD_ARGUMENT
    ok = [request()]
    assert call(ok, handle=None) == bad
    assert call(ok, view=None) == bad
    assert call(ok, n_plots=-1) == bad
    assert call(ok, capacity=-1) == bad
    assert call(None, n_plots=1) == bad
    for k in (2, 3, 4):
        assert call(ok, o=outs[:k] + [None] + outs[k + 1:]) == bad
    assert call(ok, o=[None] + outs[1:]) == bad and call(ok, o=outs[:1] + [None] + outs[2:]) == bad
    assert call(ok, craft=[n]) == bad and call(ok, craft=[-1]) == bad
    assert call([request()] * (n + 1)) == bad                                           # craft == NULL: at most one plot per craft
    assert call([request(source=0)]) == bad and call([request(source=-2)]) == bad
    assert call([request(first=1)]) == bad and call([request(count=5)]) == bad
    assert call([request(ref=-2)]) == bad and call([request(ref=s.n)]) == bad
    assert call([request(max_points=-1)]) == bad and call([request(max_points=cap + 1)]) == bad
    assert call([request(bound=3)]) == bad and call([request(bound=-1)]) == bad
    assert call([request(), request(bound=3)]) == bad                                   # one bad request refuses the whole call
    assert call([], n_plots=0) == 0 and call(None, n_plots=0, o=[None] * 5) == 0        # no plots: EPH_OK, nothing written
    assert poisoned()
    with pytest.raises(ValueError):
        batch.plot_points(views_for(s.epoch)[0], [{"source_body": 3, "start": 0.0, "end": 1.0, "tan2_angular_resolution": RES, "max_points": 4}])
    assert batch.plot_points(views_for(s.epoch)[0], []) == []
    # works, with the repeats and the order the caller asked for; rows beyond the count stay as they were
    assert call([request(ref=3), request()], craft=[2, 2]) == 0
    assert cnt[0] >= 2 and cnt[1] >= 2 and (stt[:2] == 0).all() and (cnt[2:] == -99).all()
    assert (ot[cnt[0]:cap] == -7.25).all() and (ot[2 * cap:] == -7.25).all()
    # max_points == 0 with capacity 0 and no point buffers
    assert call([request(max_points=0)], capacity=0, o=[None, None] + outs[2:]) == 0 and cnt[0] == 0 and stt[0] == 0
    # a degenerate view (everything mapped onto the camera: the error estimate is NaN) makes the reference spin forever; here the
    # search gives up and says so
    v.grid_matrix3[:] = [0.0] * 9
    v.camera_position[:] = [0.0, 0.0, 0.0]
    assert call([request()], craft=[1]) == 0
    assert stt[0] == gpu.MAX_ITERATIONS_REACHED and cnt[0] == 1
