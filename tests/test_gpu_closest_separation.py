"""-m gpu: eph_closest_separation and eph_craft_batch_closest_separation -- the app's target search (setup_target_plotting:
RelativeTrajectory::closest_separation_between + PlotSeparation.distance) -- against the Python restatement
(closest_separation_restatement.py, evaluations by the C oracle), against each other, and against the search driven from the host
over eph_craft_batch_eval. Every comparison is on bit patterns (found, time, distance, iterations, status, failed_at); there is no
tolerance anywhere."""
import ctypes as C
import importlib.util
import math

import numpy as np
import pytest

import closest_separation_restatement as cs
from conftest import ROOT, load_system
from craft_cases import DAY, SHIP, bits, gathered_knots, perturbed, propagated, snapshot_of_slabs
from ephemeris_explorer_amd.systems import load_ship, parse_epoch
from oracle import orc

pytestmark = pytest.mark.gpu

KEYS = ("found", "time", "distance", "iterations", "status", "failed_at")
INF = math.inf


def same(a, b):
    return (bool(a["found"]) == bool(b["found"]) and a["iterations"] == b["iterations"] and a["status"] == b["status"] and
            bits(a["time"]) == bits(b["time"]) and bits(a["distance"]) == bits(b["distance"]) and bits(a["failed_at"]) == bits(b["failed_at"]))


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"{what}: request {i} differs: {g} / {({k: w[k] for k in KEYS})}"


def trajectory(osol, knots, body, slice_):
    """the restatement's trajectory of one side of a host-array request"""
    if body >= 0:
        return cs.Body(osol, body)
    first, count = slice_
    return cs.Hermite(knots[0][first:first + count], knots[1][first:first + count], knots[2][first:first + count])


def restated(osol, knots, rq):
    return cs.closest_separation(trajectory(osol, knots, rq.get("source_body", -1), rq.get("source_knots", (0, 0))),
                                 trajectory(osol, knots, rq.get("target_body", -1), rq.get("target_knots", (0, 0))),
                                 rq["left"], rq["right"], rq.get("precision", 0.001), rq.get("max_iterations", 1000), rq.get("metric", 0))


def host_form(batch, nknots, crafts, targets, requests):
    """the batch form's requests as eph_closest_separation wants them, on the knots eph_craft_batch_knots gives: (requests, knots)"""
    used = sorted({int(c) for c in crafts} | {int(t) for t in targets if t >= 0})
    parts = {c: batch.knots(c, nknots[c]) for c in used}
    first, at = {}, 0
    for c in used:
        first[c] = at
        at += len(parts[c][0])
    knots = tuple(np.concatenate([parts[c][k] for c in used]) for k in range(3))
    out = []
    for c, t, rq in zip(crafts, targets, requests):
        r = {**rq, "source_knots": (first[int(c)], len(parts[int(c)][0]))}
        if t >= 0:
            r["target_knots"] = (first[int(t)], len(parts[int(t)][0]))
        out.append(r)
    return out, knots


def host_driven():
    """scripts/closest_separation_timing.py's search over eph_craft_batch_eval: the only route before this call existed"""
    spec = importlib.util.spec_from_file_location("closest_separation_timing", ROOT / "scripts" / "closest_separation_timing.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.host_driven_search


@pytest.fixture(scope="module")
def scene(gpu):
    """simple_solar_system_2433282.5 to 1951-03-01; the Mars Transfer Ship without burns for 300 days (62 103 knots) and a perturbed
    second ship, in one batch of two (the wave form)"""
    s, _, eph, osol = propagated(gpu, "simple_solar_system_2433282.5", parse_epoch("1951-03-01 00:00:00"))
    ship = load_ship(SHIP)
    assert ship.start == s.epoch
    pos, vel = perturbed(ship, 2, 20261017)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), max_knots=70000)
    batch.propagate(ship.start + 300 * DAY)
    st = batch.status()
    print("knots", st["nknots"])
    assert (st["status"] == 0).all() and 60000 < st["nknots"][0] < 65000, (st["status"], st["nknots"])
    k0, k1 = batch.knots(0, st["nknots"][0]), batch.knots(1, st["nknots"][1])
    knots = tuple(np.concatenate([a, b]) for a, b in zip(k0, k1))
    return dict(s=s, eph=eph, osol=osol, ship=ship, batch=batch, knots=knots, slices=[(0, len(k0[0])), (len(k0[0]), len(k1[0]))])


def test_host_array_form_against_the_restatement(gpu, scene):
    """1. every body as target x both metrics, body-body pairs, three windows, small iteration caps, ship-ship: all six outputs of
    every request equal the restatement's; the whole-span searches end by the precision test, not by the cap"""
    s, eph, osol, knots, (ship0, ship1) = scene["s"], scene["eph"], scene["osol"], scene["knots"], scene["slices"]
    t0 = s.epoch
    end = knots[0][ship0[1] - 1]
    whole = {"left": t0, "right": t0 + 400 * DAY}
    name = s.names.index
    requests = [{**whole, "source_knots": ship0, "target_body": b, "metric": m} for b in range(s.n) for m in (0, 1)]
    n_whole = len(requests)
    assert n_whole == 20
    for a, b in (("Earth", "Moon"), ("Mercury", "Venus"), ("Mars", "Earth")):
        requests += [{**whole, "source_body": name(a), "target_body": name(b), "metric": m} for m in (0, 1)]
    windows = [(t0, t0 + 5 * DAY), (t0 + 100 * DAY, t0 + 250 * DAY), (end - 10.0, INF)]
    for left, right in windows:
        requests += [{"left": left, "right": right, "source_knots": ship0, "target_body": name(b), "metric": m}
                     for b in ("Sun", "Earth", "Mars") for m in (0, 1)]
    requests += [{**whole, "source_knots": ship0, "target_body": name("Mars"), "max_iterations": k, "metric": m} for k in (0, 1, 5, 20) for m in (0, 1)]
    requests += [{**whole, "source_knots": ship0, "target_knots": ship1, "metric": m} for m in (0, 1)]
    requests += [{**whole, "source_knots": ship1, "target_knots": ship0}, {**whole, "source_body": name("Mars"), "target_knots": ship1},
                 {"left": -INF, "right": INF, "source_knots": ship0, "target_knots": ship0}]          # reversed, body-ship, a ship against itself
    got = gpu.closest_separation(eph, requests, knots)
    want = [restated(osol, knots, rq) for rq in requests]
    for i, (rq, w) in enumerate(zip(requests, want)):
        print(i, {k: v for k, v in rq.items() if k not in ("left", "right")}, w["found"], w["iterations"], w["status"], w["time"], w["distance"])
        if rq.get("max_iterations", 1000) == 1000:                   # a test in which everything runs into the cap would compare nothing
            assert w["iterations"] <= 1000, (i, w)
    assert_same(got, want, "host-array form")
    assert all(w["found"] and w["status"] == 0 and w["iterations"] <= 1000 for w in want[:n_whole])
    capped = [w["iterations"] for rq, w in zip(requests, want) if "max_iterations" in rq]
    assert capped == [1, 1, 2, 2, 6, 6, 21, 21]
    assert want[-1]["iterations"] == 1 and want[-1]["distance"] == 0.0                      # d = 0 at the first iteration
    assert all(w["found"] for w in want)


@pytest.fixture(scope="module")
def wave_case(gpu, scene):
    """a few craft (one wave per craft): six perturbed copies of the ship with its burns, 150 days"""
    s, eph = scene["s"], scene["eph"]
    ship = scene["ship"]
    n = 6
    pos, vel = perturbed(ship, n, 31)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance),
                                [ship.burn_tuples(s.names)] * n, max_knots=20000)
    batch.propagate(ship.start + 150 * DAY)
    st = batch.status()
    assert (st["status"] == 0).all()
    return dict(batch=batch, n=n, nknots=st["nknots"], span=150)


def mixed_requests(s, n, rng, count, span):
    """craft listed several times, body targets and craft targets (a craft against itself among them), both metrics, three windows
    (span: the days the craft cover)"""
    t0 = s.epoch
    windows = [(t0, t0 + 400 * DAY), (t0 + 0.25 * span * DAY, t0 + 0.75 * span * DAY), (-INF, INF)]
    crafts = np.concatenate([[0, 0, n - 1, n - 1], rng.integers(0, n, count)])
    targets = np.concatenate([[0, -1, n - 1, 0], np.where(rng.random(count) < 0.5, rng.integers(0, n, count), -1)])
    requests = []
    for p in range(len(crafts)):
        left, right = windows[p % 3]
        requests.append({"left": left, "right": right, "metric": p % 2, "target_body": int(rng.integers(0, s.n)) if targets[p] < 0 else -1})
    return crafts, targets, requests


def test_batch_form_wave(gpu, scene, wave_case):
    """2a. the wave form: equal to the host-array form on eph_craft_batch_knots, and to the restatement"""
    s, eph, osol = scene["s"], scene["eph"], scene["osol"]
    batch, n, nknots = wave_case["batch"], wave_case["n"], wave_case["nknots"]
    crafts, targets, requests = mixed_requests(s, n, np.random.default_rng(3), 60, wave_case["span"])
    got = batch.closest_separation(requests, craft=crafts, target_craft=targets)
    host_requests, knots = host_form(batch, nknots, crafts, targets, requests)
    assert_same(got, gpu.closest_separation(eph, host_requests, knots), "batch form against the host-array form")
    want = [restated(osol, knots, rq) for rq in host_requests]
    assert_same(got, want, "batch form against the restatement")
    assert got[0]["found"] and got[0]["iterations"] == 1 and got[0]["distance"] == 0.0      # craft 0 against itself
    assert all(w["iterations"] <= 1000 for w in want) and sum(w["found"] for w in want) > 50
    # craft == NULL: request p is craft p; one dict for all
    rq = {"left": s.epoch, "right": s.epoch + 400 * DAY, "target_body": s.names.index("Mars")}
    per_craft = batch.closest_separation(rq)
    listed = batch.closest_separation([rq] * n, craft=np.arange(n))
    assert len(per_craft) == n
    assert_same(per_craft, listed, "craft == NULL")
    assert_same(per_craft, [restated(osol, batch.knots(c), {**rq, "source_knots": (0, int(nknots[c]))}) for c in range(n)], "craft == NULL, restated")


@pytest.fixture(scope="module")
def thread_case(gpu, scene):
    """the thread form with dealt lanes: 16 384 perturbed copies of the ship with its burns over the first 1.5 days, max_knots = 4096"""
    s, eph, ship = scene["s"], scene["eph"], scene["ship"]
    n = 16384
    pos, vel = perturbed(ship, n, 20261017)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance),
                                [ship.burn_tuples(s.names)] * n, max_knots=4096)
    batch.propagate(ship.start + 1.5 * DAY)
    st = batch.status()
    assert (st["status"] == 0).all()
    return dict(batch=batch, n=n, nknots=st["nknots"], span=1.5)


def test_batch_form_thread_dealt_lanes(gpu, scene, thread_case):
    """2b. 16 384 craft dealt to the lanes: every craft against the Earth, and a shuffled list with repeats, craft targets and
    self-targets, against the host-array form on the knots read back; every 64th craft against the restatement"""
    s, eph, osol = scene["s"], scene["eph"], scene["osol"]
    batch, n, nknots = thread_case["batch"], thread_case["n"], thread_case["nknots"]
    assert n > 12288
    knots, first, count = gathered_knots(batch, nknots)
    sliced = lambda c: (int(first[c]), int(count[c]))                                       # noqa: E731
    rq = {"left": s.epoch, "right": s.epoch + 400 * DAY, "target_body": s.names.index("Earth")}
    got = batch.closest_separation(rq)
    assert len(got) == n
    assert_same(got, gpu.closest_separation(eph, [{**rq, "source_knots": sliced(c)} for c in range(n)], knots), "every craft against the Earth")
    for c in range(0, n, 64):
        assert same(got[c], restated(osol, knots, {**rq, "source_knots": sliced(c)})), c
    assert all(g["found"] and g["status"] == 0 and g["iterations"] <= 1000 for g in got)
    rng = np.random.default_rng(5)
    crafts, targets, requests = mixed_requests(s, n, rng, 3000, thread_case["span"])
    crafts, targets = np.concatenate([crafts, [7, 7, 7]]), np.concatenate([targets, [7, 9000, -1]])
    requests += [{"left": s.epoch, "right": INF, "target_body": -1}] * 2 + [{"left": s.epoch, "right": INF, "target_body": 0}]
    mixed = batch.closest_separation(requests, craft=crafts, target_craft=targets)
    host_requests = [{**r, "source_knots": sliced(c), **({"target_knots": sliced(t)} if t >= 0 else {})} for c, t, r in zip(crafts, targets, requests)]
    assert_same(mixed, gpu.closest_separation(eph, host_requests, knots), "a shuffled list with repeats and craft targets")
    for p in range(0, len(crafts), 16):
        assert same(mixed[p], restated(osol, knots, host_requests[p])), p
    assert sum(g["found"] for g in mixed) > 2000


def test_host_driven_search_over_craft_batch_eval(gpu, scene, wave_case, thread_case):
    """3. metric 0, body targets: the search driven from the host over eph_craft_batch_eval(per_craft = 1, reference_body = B) -- the
    only route before this call -- gives the same times and iteration counts (and every other output)"""
    s, eph = scene["s"], scene["eph"]
    search = host_driven()
    for case, bodies_of in ((wave_case, lambda n: [s.names.index(x) for x in ("Mars", "Earth", "Sun", "Moon", "Venus", "Mars")]),
                            (thread_case, lambda n: np.where(np.arange(n) % 3 == 0, s.names.index("Moon"), s.names.index("Earth")))):
        batch, n = case["batch"], case["n"]
        bodies = bodies_of(n)
        for left, right in ((s.epoch, s.epoch + 400 * DAY), (s.epoch + 0.25 * case["span"] * DAY, s.epoch + 0.75 * case["span"] * DAY)):
            got = batch.closest_separation([{"left": left, "right": right, "target_body": int(b)} for b in bodies])
            want = search(batch, eph, bodies, left, right)
            assert want["evals"] >= 2
            for k in KEYS:
                g = np.array([x[k] for x in got], dtype=want[k].dtype)
                assert g.tobytes() == want[k].tobytes(), (k, n, np.flatnonzero(g != want[k])[:5])
            assert all(x["found"] for x in got)


def test_the_batch_is_untouched(gpu, scene):
    """4. summary, knot slabs, events and a following propagate are bit-equal with and without a search in between; a clone answers
    alike"""
    from ephemeris_explorer_amd.systems import soi_radii
    s, eph, ship = scene["s"], scene["eph"], scene["ship"]
    n = 40
    pos, vel = perturbed(ship, n, 11)
    burns = ship.burn_tuples(s.names)
    mid, end = ship.start + 20 * DAY, ship.start + 30 * DAY
    a, b = (gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), [burns] * n,
                                max_knots=20000).enable_events(soi_radii(s)) for _ in range(2))
    a.propagate(mid)
    b.propagate(mid)
    before = snapshot_of_slabs(a)
    crafts, targets, requests = mixed_requests(s, n, np.random.default_rng(4), 200, 20)
    got = a.closest_separation(requests, craft=crafts, target_craft=targets)
    assert snapshot_of_slabs(a) == before == snapshot_of_slabs(b)
    assert_same(a.clone().closest_separation(requests, craft=crafts, target_craft=targets), got, "clone")
    assert_same(b.closest_separation(requests, craft=crafts, target_craft=targets), got, "the twin")
    assert sum(g["found"] for g in got) > 100
    a.propagate(end)
    b.propagate(end)
    assert snapshot_of_slabs(a) == snapshot_of_slabs(b)


def test_live_table(gpu):
    """5. a search whose window runs past the table's end stops at the target's end; after eph_ephemeris_append the same call
    searches further; both equal the restatement on the respective table"""
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
    mars = s.names.index("Mars")
    rq = {"left": s.epoch, "right": s.epoch + 400 * DAY, "target_body": mars}
    knots = [batch.knots(c) for c in range(n)]
    want_for = lambda table: [restated(table, knots[c], {**rq, "source_knots": (0, len(knots[c][0]))}) for c in range(n)]   # noqa: E731
    long_ = batch.closest_separation(rq)
    assert_same(long_, want_for(olive), "the whole table")
    cut = max(pieces[1][1].info(b)[0] for b in range(s.n))
    eph.clear_after(cut)
    olive.clear_after(cut)
    ref_end = olive.info(mars)[0] + olive.info(mars)[1] * float(olive.info(mars)[2])
    assert s.epoch + 100 * DAY <= ref_end < min(k[0][-1] for k in knots)
    short = batch.closest_separation(rq)
    assert_same(short, want_for(olive), "the table cut short")
    assert all(x["found"] and x["time"] <= ref_end for x in short)
    eph.append(pieces[1][0])
    assert olive.append(pieces[1][1])
    again = batch.closest_separation(rq)
    assert_same(again, want_for(olive), "the table grown again")
    assert_same(again, long_, "the table as it was")


def test_drained_batches(gpu, scene):
    """6. after eph_craft_batch_reset_knots only the drained slab's span is searched; a craft with one knot gives found 0, EPH_OK"""
    s, eph, osol, ship = scene["s"], scene["eph"], scene["osol"], scene["ship"]
    n = 5
    pos, vel = perturbed(ship, n, 12)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, gpu.AdaptiveParams.default(ship.tolerance), max_knots=20000)
    rq = {"left": -INF, "right": INF, "target_body": s.names.index("Moon")}
    none = dict(found=False, time=0.0, distance=0.0, iterations=0, status=0, failed_at=0.0)
    assert_same(batch.closest_separation(rq), [none] * n, "one knot")
    batch.propagate(ship.start + 3 * DAY)
    last = [batch.knots(c)[0][-1] for c in range(n)]
    batch.reset_knots()
    assert_same(batch.closest_separation(rq), [none] * n, "one knot again")
    batch.propagate(ship.start + 6 * DAY)
    got = batch.closest_separation(rq)
    crafts, targets = np.arange(n), np.array([1, 2, 3, 4, 0])
    pairs = batch.closest_separation([{**rq, "target_body": -1}] * n, craft=crafts, target_craft=targets)
    nk = batch.status()["nknots"]
    assert (nk >= 2).all()
    for c in range(n):
        k = batch.knots(c)
        assert k[0][0] == last[c]
        assert same(got[c], restated(osol, k, {**rq, "source_knots": (0, len(k[0]))})), c
        assert got[c]["found"] and got[c]["time"] >= last[c]
    host_requests, knots = host_form(batch, nk, crafts, targets, [{**rq, "target_body": -1}] * n)
    assert_same(pairs, [restated(osol, knots, r) for r in host_requests], "craft pairs on drained slabs")


def test_failure_statuses_and_refusals(gpu, scene):
    """7. EPH_EVAL_FAILED through an empty knot slice and through a NaN distance difference, with the restatement's failed_at; every
    refusal returns EPH_ERR_BAD_ARGUMENT and leaves poisoned outputs poisoned"""
    s, eph, osol, knots, (ship0, ship1) = scene["s"], scene["eph"], scene["osol"], scene["knots"], scene["slices"]
    t0 = s.epoch
    failing = [{"left": t0, "right": t0 + 400 * DAY, "source_knots": ship0, "target_knots": (5, 0), "metric": 1},
               {"left": t0, "right": t0 + 400 * DAY, "source_knots": (0, 0), "target_body": 3},
               {"left": -INF, "right": INF, "source_knots": (0, 0), "target_knots": (0, 0)},
               {"left": t0 + DAY, "right": t0 + 2 * DAY, "source_body": 4, "target_knots": (ship1[0], 0)}]
    # a NaN difference of the two distances (two knots at an infinite position: inf - inf inside the segment): the one deliberate
    # departure from the reference, EVAL_FAILED at mid1
    n_all = len(knots[0])
    knots = (np.concatenate([knots[0], [t0, t0 + 3000.0]]), np.concatenate([knots[1], [[INF, 0.0, 0.0]] * 2]), np.concatenate([knots[2], np.zeros((2, 3))]))
    failing.append({"left": -INF, "right": INF, "source_knots": (n_all, 2), "target_body": 3})
    got = gpu.closest_separation(eph, failing, knots)
    want = [restated(osol, knots, rq) for rq in failing]
    assert_same(got, want, "empty knot slices, a NaN difference")
    assert all(g["status"] == gpu.EVAL_FAILED and not g["found"] and g["iterations"] == 1 for g in got)
    assert got[4]["failed_at"] == t0 + 3000.0 / 3.0
    assert got[0]["failed_at"] == t0 + (knots[0][ship0[1] - 1] - t0) / 3.0 and got[3]["failed_at"] == (t0 + DAY) + DAY / 3.0
    # refusals
    L = gpu._lib()
    bad = gpu.ERR_BAD_ARGUMENT
    R = gpu.SeparationRequest
    dp, u8p, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    m = 4
    found = np.full(m, 0xA5, np.uint8)
    time, dist, fail = np.full(m, -7.25), np.full(m, -7.25), np.full(m, -7.25)
    it, st = np.full(m, -99, np.int32), np.full(m, -99, np.int32)
    outs = [found.ctypes.data_as(u8p), time.ctypes.data_as(dp), dist.ctypes.data_as(dp), it.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
            fail.ctypes.data_as(dp)]

    def poisoned():
        return ((found == 0xA5).all() and (time == -7.25).all() and (dist == -7.25).all() and (fail == -7.25).all() and (it == -99).all() and
                (st == -99).all())

    kt, kp, kv = (np.ascontiguousarray(k[:100]) for k in knots)
    nk = len(kt)

    def request(source=-1, target=3, sk=(0, 50), tk=(0, 0), left=t0, right=t0 + DAY, precision=0.001, max_iterations=1000, metric=0):
        return R(source, target, sk[0], sk[1], tk[0], tk[1], left, right, precision, max_iterations, metric)

    def call(rqs, n_requests=None, handle=eph._h, n_knots=nk, arrays=(kt, kp, kv), o=outs):
        arr = (R * max(len(rqs), 1))(*rqs) if rqs is not None else None
        ptrs = [None if a is None else a.ctypes.data_as(dp) for a in arrays]
        return L.eph_closest_separation(handle, len(rqs) if n_requests is None else n_requests, arr, n_knots, *ptrs, *o)
    ok = [request()]
    assert call(ok, handle=None) == bad
    assert call(ok, n_requests=-1) == bad and call(ok, n_knots=-1) == bad
    assert call(None, n_requests=1) == bad
    for k in range(6):
        assert call(ok, o=outs[:k] + [None] + outs[k + 1:]) == bad
    for k in range(3):
        assert call(ok, arrays=[None if j == k else a for j, a in enumerate((kt, kp, kv))]) == bad
    assert call([request(source=s.n)]) == bad and call([request(source=-2)]) == bad
    assert call([request(target=s.n)]) == bad and call([request(target=-2)]) == bad
    assert call([request(sk=(-1, 5))]) == bad and call([request(sk=(0, -1))]) == bad and call([request(sk=(60, 41))]) == bad
    assert call([request(sk=(nk + 1, 0))]) == bad and call([request(sk=(1, 2**62))]) == bad
    assert call([request(target=-1, tk=(90, 11))]) == bad and call([request(target=-1, tk=(-1, 2))]) == bad
    assert call([request(metric=2)]) == bad and call([request(metric=-1)]) == bad
    assert call([request(left=math.nan)]) == bad and call([request(right=math.nan)]) == bad
    assert call([request(max_iterations=-1)]) == bad and call([request(max_iterations=2**20 + 1)]) == bad
    assert call([request(), request(metric=2)]) == bad                                  # one bad request refuses the whole call
    assert call([], n_requests=0) == 0 and call(None, n_requests=0, o=[None] * 6) == 0  # no requests: EPH_OK, nothing written
    assert poisoned()
    assert gpu.closest_separation(eph, []) == []
    # a body's knot fields are not read; the cap itself and a NaN or zero precision are accepted and end
    assert call([request(sk=(0, 50), target=3, tk=(-5, 2**62)), request(max_iterations=2**20, precision=math.nan, right=t0 + 100.0),
                 request(max_iterations=50, precision=0.0)]) == 0
    assert (st[:3] == 0).all() and (found[:3] == 1).all() and it[1] == 2**20 + 1 and it[2] <= 51 and st[3] == -99 and found[3] == 0xA5
    # ---- the batch form
    found[:], time[:], dist[:], fail[:], it[:], st[:] = 0xA5, -7.25, -7.25, -7.25, -99, -99
    batch = scene["batch"]
    n = batch.n
    assert n == 2

    def brequest(source=-1, target=3, sk=(0, 0), tk=(0, 0), **kw):
        return request(source=source, target=target, sk=sk, tk=tk, **kw)

    def bcall(rqs, n_requests=None, handle=batch._h, craft=None, target_craft=None, o=outs):
        arr = (R * max(len(rqs), 1))(*rqs) if rqs is not None else None
        cr = None if craft is None else np.asarray(craft, dtype=np.int64)
        tg = None if target_craft is None else np.asarray(target_craft, dtype=np.int64)
        return L.eph_craft_batch_closest_separation(handle, len(rqs) if n_requests is None else n_requests, arr,
                                                    None if cr is None else cr.ctypes.data_as(i64p), None if tg is None else tg.ctypes.data_as(i64p), *o)
    ok = [brequest()]
    assert bcall(ok, handle=None) == bad
    assert bcall(ok, n_requests=-1) == bad
    assert bcall(None, n_requests=1) == bad
    for k in range(6):
        assert bcall(ok, o=outs[:k] + [None] + outs[k + 1:]) == bad
    assert bcall(ok, craft=[n]) == bad and bcall(ok, craft=[-1]) == bad
    assert bcall([brequest(target=-1)], target_craft=[n]) == bad
    assert bcall([brequest()] * (n + 1)) == bad                                          # craft == NULL: at most one request per craft
    assert bcall([brequest(source=0)]) == bad and bcall([brequest(source=-2)]) == bad
    assert bcall([brequest(sk=(1, 0))]) == bad and bcall([brequest(sk=(0, 5))]) == bad
    assert bcall([brequest(tk=(1, 0))]) == bad and bcall([brequest(tk=(0, 5))]) == bad
    assert bcall([brequest(target=-2)]) == bad and bcall([brequest(target=s.n)]) == bad
    assert bcall([brequest(target=-1)]) == bad and bcall([brequest(target=-1)], target_craft=[-1]) == bad      # the target given neither way
    assert bcall([brequest(target=3)], target_craft=[1]) == bad                          # ... and both ways
    assert bcall([brequest(metric=2)]) == bad and bcall([brequest(metric=-1)]) == bad
    assert bcall([brequest(left=math.nan)]) == bad and bcall([brequest(right=math.nan)]) == bad
    assert bcall([brequest(max_iterations=-1)]) == bad and bcall([brequest(max_iterations=2**20 + 1)]) == bad
    assert bcall([brequest(), brequest(metric=2)]) == bad
    assert bcall([], n_requests=0) == 0 and bcall(None, n_requests=0, o=[None] * 6) == 0
    assert poisoned()
    with pytest.raises(ValueError):
        batch.closest_separation([{"source_body": 3, "left": 0.0, "right": 1.0, "target_body": 0}])
    assert batch.closest_separation([]) == []
    # works, with the repeats and the order the caller asked for; entries beyond the requests stay as they were
    assert bcall([brequest(target=-1), brequest(target=5), brequest(target=-1)], craft=[1, 1, 0], target_craft=[0, -1, 0]) == 0
    assert (st[:3] == 0).all() and (found[:3] == 1).all() and st[3] == -99 and found[3] == 0xA5 and it[2] == 1 and dist[2] == 0.0
