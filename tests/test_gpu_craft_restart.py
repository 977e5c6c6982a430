"""-m gpu: eph_craft_batch_restart -- flight-plan restart of a spacecraft batch in place -- against the CPU oracle.

The expected value of every craft is the app's own flow restated on the oracle: orc.Craft propagated with the old plan, the restart
epoch from pyoracle.timeline_divergence_time_before (max'ed with the trajectory start), the knot at exactly that epoch, a NEW orc.Craft
from that knot with the new plan, and the two solutions merged with pyoracle.hermite_join / transitions_join / apsides_join
(PredictionTarget::merge). Every comparison is on bit patterns; there is no tolerance anywhere."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_system
from craft_cases import DAY, SHIP, bits, perturbed, same, simple_system, snapshot_of_knots  # noqa: F401  (the fixture)
from ephemeris_explorer_amd.systems import load_ship, parse_epoch, soi_radii
from oracle import orc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

T1 = parse_epoch("1950-08-01 00:00:00")
T2 = parse_epoch("1950-08-20 00:00:00")
EVENTS_FULL = 7


def edit(burns, e):
    """the issue's six plan edits (e = craft % 6): (new burns, plan_end or None)"""
    b = list(burns)
    if e in (0, 1):                                          # burn 3 / burn 4 1 % stronger
        s, en, a, r = b[e + 2]
        b[e + 2] = (s, en, np.asarray(a) * 1.01, r)
    elif e == 3:                                             # the first burn's z component
        s, en, a, r = b[0]
        a = np.array(a, dtype=np.float64)
        a[2] = 0.0101
        b[0] = (s, en, a, r)
    elif e == 4:                                             # an extra inertial burn
        t = parse_epoch("1950-03-15 00:00:00")
        b.append((t, t + 120.0, np.array([1e-3, 0.0, 0.0]), -1))
    return b, (parse_epoch("1950-02-01 00:00:00") if e == 5 else None)


def edits(burns, n):
    plans = [edit(burns, c % 6) for c in range(n)]
    ends = np.array([np.inf if p[1] is None else p[1] for p in plans])
    return [p[0] for p in plans], ends


def restart_epoch(kt, old, new, plan_end, params_changed=False):
    """flight_plan.rs:283-292 on the oracle's knots"""
    if params_changed:
        return kt[0]
    before = kt[-1] if not np.isfinite(plan_end) else min(plan_end, kt[-1])
    d = po.timeline_divergence_time_before(new, old, before)
    assert d is not None
    return max(d, kt[0])


def restart_from(c, osol, mu, method, tol, old, new, plan_end, t2, soi=None, params_changed=False, new_tol=None):
    """the second half of the app's flow: restart epoch, exact knot, a new orc.Craft from it to t2, merged"""
    kt, kp, kv = c.knots()
    steps1 = c.state()["steps"]
    epoch = restart_epoch(kt, old, new, plan_end, params_changed)
    hit = np.flatnonzero(kt == epoch)
    assert len(hit) == 1, "the oracle has no knot at the restart epoch"
    j = int(hit[0])
    t = tol if new_tol is None else new_tol
    c2 = orc.Craft(osol, mu, epoch, kp[j], kv[j], method, tol_pos=t, tol_vel=t, burns=new, soi_radius=soi)
    st = c2.step_to(t2)
    nt, npos, nvel = c2.knots()
    s2 = c2.state()
    out = dict(epoch=epoch, j=j, status=st, state=s2, steps=steps1 + s2["steps"],
               knots=(np.concatenate([kt[:j], nt]), np.concatenate([kp[:j], npos]), np.concatenate([kv[:j], nvel])))
    assert len(out["knots"][0]) == len(po.hermite_join(list(zip(kt, kp, kv)), list(zip(nt, npos, nvel))))
    if soi is not None:
        out["tr"] = po.transitions_join(list(zip(*c.transitions())), list(zip(*c2.transitions())), epoch)
        out["ap"] = po.apsides_join(list(zip(*c.apsides())), list(zip(*c2.apsides())), epoch)
    return out


def oracle_flow(osol, mu, t0, pos, vel, method, tol, old, new, plan_end, t1, t2, soi=None, new_tol=None):
    c = orc.Craft(osol, mu, t0, pos, vel, method, tol_pos=tol, tol_vel=tol, burns=old, soi_radius=soi)
    assert c.step_to(t1) == 0
    return restart_from(c, osol, mu, method, tol, old, new, plan_end, t2, soi, params_changed=new_tol is not None and new_tol != tol,
                        new_tol=new_tol)


def check_craft(batch, i, want, what, st=None, gs=None, counts=None, knots=None):
    st = batch.status() if st is None else st
    gs = batch.state() if gs is None else gs
    cs = want["state"]
    assert st["status"][i] == want["status"], f"{what}: status {st['status'][i]} vs {want['status']}"
    assert st["attempts"][i] == cs["attempts"], f"{what}: attempts {st['attempts'][i]} vs {cs['attempts']}"
    assert st["steps"][i] == want["steps"], f"{what}: steps {st['steps'][i]} vs {want['steps']}"
    assert bits(gs["t"][i]) == bits(cs["t"]), f"{what}: time {gs['t'][i]!r} vs {cs['t']!r}"
    assert same(gs["pos"][i], cs["pos"]) and same(gs["vel"][i], cs["vel"]), f"{what}: state"
    assert bits(gs["next_h"][i]) == bits(cs["next_h"]), f"{what}: next_h {gs['next_h'][i]!r} vs {cs['next_h']!r}"
    kt, kp, kv = batch.knots(i, st["nknots"][i]) if knots is None else knots
    wt, wp, wv = want["knots"]
    assert len(kt) == len(wt), f"{what}: {len(kt)} vs {len(wt)} knots"
    assert same(kt, wt) and same(kp, wp) and same(kv, wv), f"{what}: knots differ"
    if "tr" in want:
        (tt, tb), ap = batch.events(i, counts)
        check_events(((tt, tb), ap), want, what)


def check_events(got, want, what):
    (tt, tb), (at, ad, ab, ak) = got
    assert same(tt, [x[0] for x in want["tr"]]) and np.array_equal(tb, [x[1] for x in want["tr"]]), f"{what}: transitions"
    wa = want["ap"]
    assert len(at) == len(wa), f"{what}: {len(at)} vs {len(wa)} apsides"
    assert same(at, [x[0] for x in wa]) and same(ad, [x[1] for x in wa]), f"{what}: apsis times / distances"
    assert np.array_equal(ab, [x[2] for x in wa]) and np.array_equal(ak, [x[3] for x in wa]), f"{what}: apsis bodies / kinds"


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def restart_epochs_pyoracle(batch, crafts, old, news, ends):
    """restart_epoch per craft from the batch's own (undrained) knots and pyoracle"""
    out = []
    for c in crafts:
        kt = batch.knots(int(c))[0]
        out.append(restart_epoch(kt, old, news[c], ends[c]))
    return np.array(out)


def test_wave_form_with_events(gpu, simple_system):
    """1. 192 craft (wave form), events on: to 1950-08-01, restart with the six edits, to 1950-08-20; every craft's knots, state,
    next_h, status, attempts, steps, transitions and apsides equal the oracle's merged flow, and restart_epoch equals pyoracle's."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    soi = soi_radii(s)
    n = 192
    pos, vel = perturbed(ship, n, 20261016)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000).enable_events(soi)
    batch.propagate(T1)
    assert (batch.status()["status"] == 0).all()
    want_epoch = restart_epochs_pyoracle(batch, range(n), old, news, ends)
    epoch, outcome = batch.restart(news, plan_end=ends)
    assert (outcome == 0).all(), np.unique(outcome, return_counts=True)
    assert same(epoch, want_epoch)
    # the issue's table of restart epochs (days after the ship's start, to 1e-4 d)
    days = np.round((epoch[:6] - ship.start) / DAY, 4)
    assert days.tolist() == [58.1753, 207.6556, 207.6592, 0.0106, 58.1760, 0.0345]
    batch.propagate(T2)
    st, gs, counts = batch.status(), batch.state(), batch.event_counts()
    assert (counts[2] == 0).all()
    for c in range(n):
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, news[c], ends[c], T1, T2, soi)
        assert bits(want["epoch"]) == bits(epoch[c])
        assert 2 <= len(want["tr"]) <= 4
        check_craft(batch, c, want, f"craft {c} (edit {c % 6})", st, gs, counts)


def test_thread_form_dealt_lanes(gpu, simple_system):
    """2. 16 384 copies (thread form, dealt to the lanes) to ship start + 220 d, restart, to 1950-08-20: a 512-craft sample against the
    oracle; ALL craft against a fresh batch created from each craft's restart knot with the new burns (knots from j on, summary
    records except steps; steps differ by the steps taken before the restart = the old knot count minus one)."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 16384
    pos, vel = perturbed(ship, n, 20261017)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    t1 = ship.start + 220 * DAY
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=8192)
    batch.propagate(t1)
    st1 = batch.status()
    assert (st1["status"] == 0).all()
    crafts = np.unique(np.concatenate([[0], np.random.default_rng(43).choice(n, 511, replace=False)]))
    want_epoch = restart_epochs_pyoracle(batch, crafts, old, news, ends)
    epoch, outcome = batch.restart(news, plan_end=ends)
    assert (outcome == 0).all(), np.unique(outcome, return_counts=True)
    assert same(epoch[crafts], want_epoch)
    j = batch.status()["nknots"] - 1                         # join: knots 0 .. j stay
    y, inside = batch.eval(epoch[None, :], raw=True)         # knot j itself
    assert inside.all()
    fresh = gpu.SpacecraftBatch(eph, epoch, y[0, :3].T, y[0, 3:].T, ship.integrator, params, news, max_knots=8192)
    batch.propagate(T2)
    fresh.propagate(T2)
    rec, frec = batch.summary(), fresh.summary()
    assert (rec["status"] == 0).all() and (frec["status"] == 0).all()
    for f in ("t", "pos", "vel", "next_h", "status", "attempts"):
        assert np.array_equal(raw(rec[f]), raw(frec[f])), f
    assert np.array_equal(rec["nknots"], j + frec["nknots"])
    assert np.array_equal(rec["steps"] - frec["steps"], st1["nknots"] - 1) and np.array_equal(st1["steps"], st1["nknots"] - 1)
    # the restarted slab from j on = the fresh slab: the fresh knots' epochs evaluated on the restarted batch return its knots
    nkf = frec["nknots"].astype(np.int64)
    rows = 256
    for r0 in range(0, int(nkf.max()), rows):
        m = min(rows, int(nkf.max()) - r0)
        ft, fy = fresh.knot_slabs(r0, m)
        live = (r0 + np.arange(m))[:, None] < nkf[None, :]
        at = np.where(live, ft, ft[0][None, :])
        gy, gin = batch.eval(at, raw=True)
        assert gin[live].all()
        assert np.array_equal(bits(gy)[np.broadcast_to(live[:, None, :], gy.shape)], bits(fy)[np.broadcast_to(live[:, None, :], fy.shape)]), r0
    gs, st = batch.state(), batch.status()
    for c in crafts:
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, news[c], ends[c], t1, T2)
        check_craft(batch, int(c), want, f"craft {c} (edit {c % 6})", st, gs)


@pytest.mark.parametrize("method", ["DormandPrince54", "Fine45"])
def test_fsal_and_nystrom_forms(gpu, simple_system, method):
    """3. FSAL (DormandPrince54) and ERKNG (Fine45) batches: the FSAL stage registers of the old propagator must not reach the first
    step after the restart (from_problem sets them from the state)."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 12
    pos, vel = perturbed(ship, n, 31)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    t1, t2 = ship.start + 70 * DAY, ship.start + 75 * DAY
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, method, params, [old] * n, max_knots=20000)
    batch.propagate(t1)
    assert (batch.status()["status"] == 0).all()
    epoch, outcome = batch.restart(news, plan_end=ends)
    assert (outcome == 0).all()
    batch.propagate(t2)
    for c in range(n):
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], method, ship.tolerance, old, news[c], ends[c], t1, t2)
        assert bits(want["epoch"]) == bits(epoch[c])
        check_craft(batch, c, want, f"{method} craft {c} (edit {c % 6})")


def test_subset_and_clones(gpu, simple_system):
    """4. `which` = every third craft: the others stay bit-identical to a clone that was not restarted, after the same propagate;
    restarting a clone leaves the original unchanged."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    soi = soi_radii(s)
    n = 30
    pos, vel = perturbed(ship, n, 41)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    t1, t2 = ship.start + 70 * DAY, ship.start + 90 * DAY
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000).enable_events(soi)
    batch.propagate(t1)
    keep = batch.clone()
    other = batch.clone()
    before = snapshot_of_knots(batch)
    # a clone restarted: the original is unchanged
    scratch = batch.clone()
    e_all, o_all = scratch.restart(news, plan_end=ends)
    assert (o_all == 0).all()
    del scratch
    assert snapshot_of_knots(batch) == before
    sel = np.arange(n) % 3 == 0
    epoch, outcome = batch.restart(news, plan_end=ends, which=sel)
    assert (outcome[sel] == 0).all() and (outcome[~sel] == gpu.SpacecraftBatch.UNSELECTED).all()
    assert np.isnan(epoch[~sel]).all() and same(epoch[sel], e_all[sel])
    e_idx, o_idx = other.restart(news, plan_end=ends, which=np.flatnonzero(sel))   # indices select the same craft
    assert np.array_equal(o_idx, outcome) and same(e_idx[sel], epoch[sel])
    batch.propagate(t2)
    keep.propagate(t2)
    rec, krec = batch.summary(), keep.summary()
    assert rec[~sel].tobytes() == krec[~sel].tobytes()
    counts, kcounts = batch.event_counts(), keep.event_counts()
    for c in np.flatnonzero(~sel):
        assert all(same(a, b) for a, b in zip(batch.knots(int(c)), keep.knots(int(c)))), c
        got, ref = batch.events(int(c), counts), keep.events(int(c), kcounts)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for pa, pb in zip(got, ref) for a, b in zip(pa, pb)), c
    st, gs = batch.status(), batch.state()
    for c in np.flatnonzero(sel):
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, news[c], ends[c], t1, t2, soi)
        check_craft(batch, int(c), want, f"selected craft {c}", st, gs, counts)


def test_drains(gpu, simple_system):
    """5. (a) drained at T1, then edit 3: no knot at the restart epoch -- EPH_EVAL_FAILED, the craft unchanged (summary, slab, events,
    and its timeline: it propagates on exactly as an unrestarted clone). (b) drained at day 100, propagated to T1, then edit 1:
    restarted; the caller's host history joined at the returned epoch equals the oracle."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    soi = soi_radii(s)
    n = 6
    pos, vel = perturbed(ship, n, 51)
    old = ship.burn_tuples(s.names)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    plan3 = [edit(old, 3)[0]] * n
    a = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000).enable_events(soi)
    a.propagate(T1)
    full_knots = [a.knots(c)[0] for c in range(n)]
    a.reset_knots()
    keep = a.clone()
    before = snapshot_of_knots(a)
    epoch, outcome = a.restart(plan3)
    assert (outcome == gpu.EVAL_FAILED).all()
    assert same(epoch, [restart_epoch(full_knots[c], old, plan3[c], np.inf) for c in range(n)])
    assert snapshot_of_knots(a) == before
    a.propagate(T1 + 2 * DAY)
    keep.propagate(T1 + 2 * DAY)
    assert snapshot_of_knots(a) == snapshot_of_knots(keep)
    # (b)
    plan1 = [edit(old, 1)[0]] * n
    b = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000)
    b.propagate(ship.start + 100 * DAY)
    history = [b.knots(c) for c in range(n)]
    b.reset_knots()
    b.propagate(T1)
    epoch, outcome = b.restart(plan1)
    assert (outcome == 0).all()
    b.propagate(T2)
    st, gs = b.status(), b.state()
    for c in range(n):
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, plan1[c], np.inf, T1, T2)
        assert bits(want["epoch"]) == bits(epoch[c])
        ht, hp, hv = history[c]
        kt, kp, kv = b.knots(c, st["nknots"][c])
        joined = po.hermite_join(list(zip(ht, hp, hv)), list(zip(kt, kp, kv)))
        got = (np.array([k[0] for k in joined]), np.array([k[1] for k in joined]), np.array([k[2] for k in joined]))
        check_craft(b, c, want, f"drained craft {c}", st, gs, knots=got)


def test_events_lagging(gpu, simple_system):
    """6. max_transitions = 3: the search stops once a craft holds two transitions (the Earth, and its exit at day 2.5), long before
    edit 0's restart knot at day 58 -- EPH_EVENTS_FULL, the craft unchanged; after reset_events and a propagate to no later than the
    craft's time (no step, only the search) the restart is EPH_OK, and the caller's joined event history equals the oracle's."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    soi = soi_radii(s)
    n = 8
    pos, vel = perturbed(ship, n, 20261016)
    old = ship.burn_tuples(s.names)
    plan0 = [edit(old, 0)[0]] * n
    params = gpu.AdaptiveParams.default(ship.tolerance)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n,
                                max_knots=20000).enable_events(soi, max_transitions=3, max_apsides=4096)
    batch.propagate(T1)
    ntr, nap, est = batch.event_counts()
    assert (est == EVENTS_FULL).all() and (ntr == 2).all()
    before = snapshot_of_knots(batch)
    epoch, outcome = batch.restart(plan0)
    assert (outcome == EVENTS_FULL).all()
    assert snapshot_of_knots(batch) == before
    hist = [([], []) for _ in range(n)]                     # the caller's event history: (transitions, apsides) per craft

    def absorb():
        """read every craft's lists into the history (reset_events keeps the newest transition: not twice); True if any is full"""
        counts = batch.event_counts()
        for c in range(n):
            (tt, tb), ap = batch.events(c, counts)
            tr = list(zip(tt, tb))
            if hist[c][0] and tr and bits(tr[0][0]) == bits(hist[c][0][-1][0]) and tr[0][1] == hist[c][0][-1][1]:
                tr = tr[1:]
            hist[c][0].extend(tr)
            hist[c][1].extend(zip(*ap))
        return (counts[2] == EVENTS_FULL).any()

    def search_only():
        """drain, then a propagate to no later than every craft's time: no step, only the event search"""
        batch.reset_events()
        t_now, steps = batch.state()["t"], batch.status()["steps"]
        batch.propagate(t_now.min())
        assert np.array_equal(batch.status()["steps"], steps) and same(batch.state()["t"], t_now)

    assert absorb()
    assert all(abs(h[0][1][0] - ship.start - 2.5 * DAY) < 0.01 * DAY and s.names[h[0][1][1]] == "Sun" for h in hist)
    search_only()
    epoch2, outcome2 = batch.restart(plan0)
    assert (outcome2 == 0).all() and same(epoch2, epoch)
    batch.propagate(T2)
    st, gs = batch.status(), batch.state()
    for _ in range(16):                                     # the slabs fill again (Mars): drain until the search is through
        if not absorb():
            break
        search_only()
    else:
        raise AssertionError("the event search did not finish")
    for c in range(n):
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, plan0[c], np.inf, T1, T2, soi)
        check_craft(batch, c, {k: v for k, v in want.items() if k not in ("tr", "ap")}, f"lagging craft {c}", st, gs)
        tr, ap = hist[c]
        got = ((np.array([x[0] for x in tr]), np.array([x[1] for x in tr])), tuple(np.array([x[k] for x in ap]) for k in range(4)))
        check_events(got, want, f"lagging craft {c}")


def test_parameter_change(gpu, simple_system):
    """7. A new tolerance (which = NULL) restarts every craft at its creation epoch: equal to a fresh batch with the new parameters
    and burns (except steps), and to the oracle."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    n = 12
    pos, vel = perturbed(ship, n, 71)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params, tighter = gpu.AdaptiveParams.default(ship.tolerance), gpu.AdaptiveParams.default(5e-4)
    t1, t2 = ship.start + 62 * DAY, ship.start + 66 * DAY
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000)
    batch.propagate(t1)
    steps1 = batch.status()["steps"]
    epoch, outcome = batch.restart(news, plan_end=ends, params=tighter)
    assert (outcome == 0).all() and (epoch == ship.start).all()
    assert batch.status()["nknots"].tolist() == [1] * n
    fresh = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, tighter, news, max_knots=20000)
    batch.propagate(t2)
    fresh.propagate(t2)
    rec, frec = batch.summary(), fresh.summary()
    for f in ("t", "pos", "vel", "next_h", "status", "nknots", "attempts"):
        assert np.array_equal(raw(rec[f]), raw(frec[f])), f
    assert np.array_equal(rec["steps"], frec["steps"] + steps1)
    st, gs = batch.status(), batch.state()
    for c in range(n):
        assert all(same(x, y) for x, y in zip(batch.knots(c), fresh.knots(c)))
        want = oracle_flow(osol, s.mu, ship.start, pos[c], vel[c], ship.integrator, ship.tolerance, old, news[c], ends[c], t1, t2,
                           new_tol=5e-4)
        check_craft(batch, c, want, f"craft {c}, new tolerance", st, gs)


def test_live_table_flow(gpu, simple_system):
    """8. The app's live-table flow: a table that ends at day 100; the craft fail with EPH_EVAL_FAILED (sticky); a restart re-arms them
    (EPH_OK); the table grows (eph_ephemeris_append) and the restarted batch propagates as the oracle does on the whole table."""
    s = load_system("simple_solar_system_2433282.5")
    ship = load_ship(SHIP)
    g = gpu.NBodyPropagator.from_system(s)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, s.count, s.degree)
    pieces = []
    for t in (s.epoch + 100 * DAY, T2 + 10 * DAY):
        g.step_to(t)
        assert o.step_to(t) == 0
        sg, so = g.take_solution(), o.take_solution()
        for b in range(s.n):
            assert sg.info(b) == so.info(b)
        pieces.append((sg, so))
    eph, olive = gpu.Ephemeris(pieces[0][0], s.mu), pieces[0][1].clone()
    n = 6
    pos, vel = perturbed(ship, n, 81)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000)
    batch.propagate(T1)
    crafts = [orc.Craft(olive, s.mu, ship.start, pos[c], vel[c], ship.integrator, tol_pos=ship.tolerance, tol_vel=ship.tolerance,
                        burns=old) for c in range(n)]
    for c in crafts:
        assert c.step_to(T1) == orc.EVAL_FAILED
    assert (batch.status()["status"] == gpu.EVAL_FAILED).all()
    batch.propagate(T1)
    assert (batch.status()["status"] == gpu.EVAL_FAILED).all()        # sticky
    epoch, outcome = batch.restart(news, plan_end=ends)
    assert (outcome == 0).all() and (batch.status()["status"] == 0).all()
    eph.append(pieces[1][0])
    assert olive.append(pieces[1][1])
    batch.propagate(T2)
    st, gs = batch.status(), batch.state()
    for c in range(n):
        want = restart_from(crafts[c], olive, s.mu, ship.integrator, ship.tolerance, old, news[c], ends[c], T2)
        assert want["status"] == 0 and bits(want["epoch"]) == bits(epoch[c])
        check_craft(batch, c, want, f"live craft {c} (edit {c % 6})", st, gs)


def test_refusals_and_edge_cases(gpu, simple_system):
    """9. Refusals change nothing: a bad CSR, burn_ref out of range, params with which (EPH_ERR_BAD_ARGUMENT); a relative-frame burn on
    a Tsitouras75Nystrom batch (EPH_ERR_UNSUPPORTED). An empty batch is EPH_OK. A never-propagated batch restarted equals one created
    with the new burns."""
    s, sol, eph, osol = simple_system
    ship = load_ship(SHIP)
    soi = soi_radii(s)
    n = 6
    pos, vel = perturbed(ship, n, 91)
    old = ship.burn_tuples(s.names)
    news, ends = edits(old, n)
    params = gpu.AdaptiveParams.default(ship.tolerance)
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=4096).enable_events(soi)
    batch.propagate(ship.start + DAY)
    before = snapshot_of_knots(batch)
    L, h = batch._L, batch._h
    dp, i32p, i64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    off = np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int64)
    bs, be = np.full(6, ship.start + 3600.0), np.full(6, ship.start + 3700.0)
    ba = np.zeros(18)
    br = np.full(6, -1, dtype=np.int32)
    epoch = np.full(n, -7.25)
    outcome = np.full(n, 0x5A5A, dtype=np.int32)
    which = np.ones(n, dtype=np.uint8)
    tighter = gpu.AdaptiveParams.default(5e-4)

    def call(o=off, r=br, w=None, pr=None):
        return L.eph_craft_batch_restart(h, None if w is None else w.ctypes.data_as(u8p), o.ctypes.data_as(i64p), bs.ctypes.data_as(dp),
                                         be.ctypes.data_as(dp), ba.ctypes.data_as(dp), r.ctypes.data_as(i32p), None,
                                         None if pr is None else C.byref(pr), epoch.ctypes.data_as(dp), outcome.ctypes.data_as(i32p))
    bad = gpu.ERR_BAD_ARGUMENT
    assert call(o=np.array([0, 1, 2, 1, 4, 5, 6], dtype=np.int64)) == bad       # decreasing offsets
    assert call(o=np.array([-1, 1, 2, 3, 4, 5, 6], dtype=np.int64)) == bad
    assert call(r=np.array([-1, -1, s.n, -1, -1, -1], dtype=np.int32)) == bad   # a body index out of range
    assert call(r=np.array([-1, -2, -1, -1, -1, -1], dtype=np.int32)) == bad
    assert call(w=which, pr=tighter) == bad                                     # params belong to the whole batch
    assert (epoch == -7.25).all() and (outcome == 0x5A5A).all()
    assert snapshot_of_knots(batch) == before
    assert batch.params.tol_position == ship.tolerance
    # Tsitouras75Nystrom: inertial burns only, as at creation
    inertial = [[(b[0], b[1], b[2], -1) for b in old]] * n
    ny = gpu.SpacecraftBatch(eph, ship.start, pos, vel, "Tsitouras75Nystrom", params, inertial, max_knots=4096)
    ny.propagate(ship.start + 3600.0)
    nbefore = snapshot_of_knots(ny)
    with pytest.raises(gpu.EphemerisError) as e:
        ny.restart([old] * n)
    assert e.value.status == gpu.ERR_UNSUPPORTED
    assert snapshot_of_knots(ny) == nbefore
    # an empty batch
    empty = gpu.SpacecraftBatch(eph, ship.start, np.zeros((0, 3)), np.zeros((0, 3)), ship.integrator, params)
    e0, o0 = empty.restart([])
    assert e0.shape == (0,) and o0.shape == (0,)
    # never propagated: a restart is a creation with the new burns
    fresh_old = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, [old] * n, max_knots=20000).enable_events(soi)
    created = gpu.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, params, news, max_knots=20000).enable_events(soi)
    ep, oc = fresh_old.restart(news, plan_end=ends)
    assert (oc == 0).all() and (ep == ship.start).all()
    t = ship.start + 70 * DAY
    fresh_old.propagate(t)
    created.propagate(t)
    assert snapshot_of_knots(fresh_old) == snapshot_of_knots(created)


def test_cpp_example_prints_the_python_calls_bits(gpu, tmp_path):
    """10. examples/craft_restart.cpp (SpacecraftBatch::restart of include/ephemeris_amd.hpp) builds against the library alone, runs,
    and prints the bits the same Python calls give"""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_restart"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_restart.cpp"), f"-L{libdir}", "-lephemeris_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    mu = [132712440041.27942, 398600.43550702266, 4902.80011845755]
    y = [[130800.7436285839, 344339.3116943656, 136496.914202216], [-27204249.66910069, 132940582.438431, 57641619.74238631],
         [-27017766.52877057, 133253431.1006455, 57806029.23241135]]
    dy = [[-0.007799748521575531, -0.005561934613704532, -0.00225317087714714], [-29.75359910616436, -5.189518219844614, -2.251561710555783],
          [-30.64009897505477, -4.820684674596127, -2.032529075882219]]
    t0, dt, day = -252460800.0, 21600.0, 86400.0
    sol = gpu.NBodyPropagator(y, dy, mu, t0, dt, gpu.FORWARD, [12, 3, 1], [6, 7, 6]).propagate(t0 + 40.0 * day)
    eph = gpu.Ephemeris(sol, mu)
    pos = np.array([[-27204249.668775786 + 10.0 * i, 132947582.43848978, 57641619.74241204] for i in range(3)])
    vel = np.array([[-22.207539106181895, -5.189518219791726, -2.2515617105336263]] * 3)
    burn = (t0 + 0.5 * day, t0 + 0.5 * day + 300.0, np.array([0.0, 0.0, 1e-3]), 1)
    batch = gpu.SpacecraftBatch(eph, t0, pos, vel, "Verner87", gpu.AdaptiveParams.default(1e-3), [[burn]] * 3)
    batch.propagate(t0 + 2.0 * day)
    stronger = (burn[0], burn[1], np.array([0.0, 0.0, 1e-3 * 1.01]), 1)
    extra = (t0 + 1.5 * day, t0 + 1.5 * day + 120.0, np.array([1e-3, 0.0, 0.0]), -1)
    epoch, outcome = batch.restart([[stronger], [burn], [burn, extra]])
    assert (outcome == 0).all()
    batch.propagate(t0 + 3.0 * day)
    gs, st = batch.state(), batch.status()
    lines = r.stdout.splitlines()
    rs = [ln.split() for ln in lines if ln.startswith("restart ")]
    ss = [ln.split() for ln in lines if ln.startswith("state ")]
    assert len(rs) == 3 and len(ss) == 3
    for c in range(3):
        assert rs[c][3] == f"outcome={outcome[c]}" and float.fromhex(rs[c][5]) == epoch[c]
        f = ss[c]
        assert f[3] == f"status={st['status'][c]}" and f[4] == f"knots={st['nknots'][c]}"
        printed = np.array([float.fromhex(x) for x in f[5:13]])
        assert same(printed, np.concatenate([[gs["t"][c]], gs["pos"][c], gs["vel"][c], [gs["next_h"][c]]]))
    assert epoch[1] > epoch[0] and epoch[2] == burn[1]        # unchanged plan: the last coast start; the extra burn: its coast
