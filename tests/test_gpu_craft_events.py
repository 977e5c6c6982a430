"""-m gpu: the event search (k_craft_events with soi_at_except, tr_insert and ap_insert; the drain through k_craft_reset_events) on the
scenes of tests/event_scenes.py, whose docstring says which arm every scene is there for, bit for bit against orc.Craft with the
SpacecraftSolout on the oracle's copy of the same parts. The C oracle is pinned to the Python restatement on the same scenes by
tests/test_event_scenes.py; every scene's liveness predicate is asserted again here, on the oracle lists the device is compared with.
No tolerance anywhere: status, every knot and the state (to tell a wrong sweep from a wrong search), event_counts(), and every
transition's time and body and every apsis' time, distance, body and kind, of every craft.

The scenes run in this process on the wave forms (k_craft_wave + k_craft_events<true>: the batches are small) and, one child process per
form (the kernel form is read once per process; this file run as a script), on k_craft_events<false> behind k_craft_propagate with the
craft dealt to the lanes, behind k_craft_propagate undealt (craft i on lane i) and behind k_craft_queue. Only scene T (136 craft) is
large enough to be dealt; there the knots of craft i lie in column slot_of[i] of the knot slabs and its events in column i of the event
slabs. The permutation cannot be read from outside: a search that read the wrong column would report another craft's events.

The two scenes with slabs too small on purpose (F-tr, F-ap) are drained the way tests/test_gpu_craft.py::test_event_slab_overflow_is_reported
drains: read, reset_events, propagate to the same end. The lists read are merged as a caller holding the reference's types would merge
them (event_scenes.merge_transitions: SoiTransitions::insert per entry; merge_apsides: by time, an equal time overwrites) and must
equal the oracle's single run."""
import os
import subprocess
import sys

import numpy as np
import pytest

import event_scenes as evs
from conftest import ROOT
from craft_cases import bits, same
from oracle import orc

pytestmark = pytest.mark.gpu

SCENES = {sc.name: sc for sc in evs.scenes()}
DRAINED = {sc.name: sc for sc in evs.drain_scenes()}
CASES = [(name, m) for name, sc in SCENES.items() for m in sc.methods]
DRAIN_CASES = [(name, m) for name, sc in DRAINED.items() for m in sc.methods]
T_CASES = [(name, m) for name, m in CASES if name.startswith("T-")]
_oracle = {}


def oracle_results(name, method):
    """the scene on the C oracle, once per process: (results, liveness asserted); nothing changes them afterwards"""
    if (name, method) not in _oracle:
        sc = SCENES.get(name) or DRAINED[name]
        sol = orc.Solution.from_parts(*sc.table)
        res = evs.run_oracle(sc, method, sol)
        sc.liveness(sc, method, res)
        lists = [(r["craft"].transitions(), r["craft"].apsides()) for r in res]
        _oracle[(name, method)] = (res, lists, sol)
    return _oracle[(name, method)][:2]


def new_batch(ea, sc, method):
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    p = sc.params
    params = ea.AdaptiveParams(p["h_init"], p["h_max"], p["tol_pos"], p["tol_vel"], 1.0 / 5.0, 5.0 / 1.0, 9.0 / 10.0, 1_000_000)
    batch = ea.SpacecraftBatch(eph, sc.t0, sc.pos, sc.vel, method, params, sc.burns, max_knots=sc.max_knots)
    return batch.enable_events(sc.soi, max_transitions=sc.max_tr, max_apsides=sc.max_ap)


def run_calls(batch, calls):
    for what, arg in calls:
        if what == "propagate":
            batch.propagate(arg)
        else:
            batch.step_n(arg)


def compare_sweep(batch, res, what):
    """status, knots and state: a failure here is the sweep's, not the search's"""
    st, gs = batch.status(), batch.state()
    for i, r in enumerate(res):
        cs = r["craft"].state()
        assert st["status"][i] == r["status"], f"{what} craft {i}: status {st['status'][i]} vs {r['status']}"
        ot, op, ov = r["craft"].knots()
        assert st["nknots"][i] == len(ot), f"{what} craft {i}: {st['nknots'][i]} vs {len(ot)} knots"
        kt, kp, kv = batch.knots(i, st["nknots"][i])
        first = np.flatnonzero((bits(kt) != bits(ot)) | (bits(kp) != bits(op)).any(axis=1) | (bits(kv) != bits(ov)).any(axis=1))
        assert len(first) == 0, f"{what} craft {i}: knots differ from knot {first[0]} of {len(ot)} on (t = {ot[first[0]]!r})"
        assert bits(gs["t"][i]) == bits(cs["t"]) and same(gs["pos"][i], cs["pos"]) and same(gs["vel"][i], cs["vel"]), f"{what} craft {i}: state"


def compare_events(batch, lists, what):
    counts = batch.event_counts()
    ntr, nap, est = counts
    for i, ((ott, otb), (oat, oad, oab, oak)) in enumerate(lists):
        who = f"{what} craft {i}"
        assert est[i] == 0, f"{who}: event status {est[i]}"
        (tt, tb), (at, ad, ab, ak) = batch.events(i, counts)
        assert ntr[i] == len(ott), f"{who}: {ntr[i]} transitions {list(zip(tt, tb))} vs {len(ott)} {list(zip(ott, otb))}"
        assert np.array_equal(bits(tt), bits(ott)) and np.array_equal(tb, otb), f"{who}: transitions {list(zip(tt, tb))} vs {list(zip(ott, otb))}"
        assert nap[i] == len(oat), f"{who}: {nap[i]} apsides {list(zip(at, ab, ak))} vs {len(oat)} {list(zip(oat, oab, oak))}"
        assert np.array_equal(bits(at), bits(oat)) and np.array_equal(ab, oab) and np.array_equal(ak, oak), \
            f"{who}: apsides {list(zip(at, ab, ak))} vs {list(zip(oat, oab, oak))}"
        assert np.array_equal(bits(ad), bits(oad)), f"{who}: apsis distances {ad!r} vs {oad!r}"


def check_scene(ea, name, method):
    sc = SCENES[name]
    res, lists = oracle_results(name, method)
    batch = new_batch(ea, sc, method)
    run_calls(batch, sc.calls)
    compare_sweep(batch, res, f"{name} {method}")
    compare_events(batch, lists, f"{name} {method}")


def check_legs_and_clone(ea, name, method):
    """scene T in two propagate legs (the search resumes at ev_seg), and on a clone taken between them (the event slabs and the deal
    are copied)"""
    sc = SCENES[name]
    res, lists = oracle_results(name, method)
    end = sc.calls[-1][1]
    batch = new_batch(ea, sc, method)
    batch.propagate(0.4 * end)
    ntr, nap, est = batch.event_counts()
    assert (est == 0).all() and 0 < ntr.sum() < sum(len(l[0][0]) for l in lists)          # the first leg found some of them
    snap = batch.clone()
    batch.propagate(end)
    for b, what in ((batch, "two legs"), (snap, "clone")):
        if b is snap:
            b.propagate(end)
        compare_sweep(b, res, f"{name} {method} {what}")
        compare_events(b, lists, f"{name} {method} {what}")


def check_drained(ea, name, method):
    """read, reset_events, propagate to the same end, at most 100 rounds; the merged lists equal the oracle's single run. F-tr: an
    EVENTS_FULL from inside a step leaves ev_seg on that step, which is then searched again: two consecutive reads share a time that is
    not the entry reset_events kept"""
    sc = DRAINED[name]
    res, lists = oracle_results(name, method)
    end = sc.calls[-1][1]
    batch = new_batch(ea, sc, method)
    batch.propagate(end)
    compare_sweep(batch, res, f"{name} {method}")
    tr_reads, ap_reads = [[] for _ in range(sc.n)], [[] for _ in range(sc.n)]
    rounds_full = 0
    for _ in range(100):
        counts = batch.event_counts()
        for i in range(sc.n):
            (tt, tb), (at, ad, ab, ak) = batch.events(i, counts)
            assert len(tt) <= sc.max_tr and len(at) <= sc.max_ap
            tr_reads[i].append(list(zip(tt.tolist(), tb.tolist())))
            ap_reads[i].append(list(zip(at.tolist(), ad.tolist(), ab.tolist(), ak.tolist())))
        est = counts[2]
        assert set(est.tolist()) <= {0, evs.EVENTS_FULL}, est
        if not est.any():
            break
        rounds_full += 1
        batch.reset_events()
        batch.propagate(end)
    assert rounds_full >= 1 and not batch.event_counts()[2].any(), f"{name} {method}: {rounds_full} rounds, {batch.event_counts()[2]}"
    assert not batch.status()["status"].any()
    searched_twice = False
    for i, ((ott, otb), (oat, oad, oab, oak)) in enumerate(lists):
        who = f"{name} {method} craft {i}"
        mt = evs.merge_transitions(tr_reads[i])
        assert same([x[0] for x in mt], ott) and [x[1] for x in mt] == otb.tolist(), f"{who}: merged {mt} vs {list(zip(ott, otb))}\nreads {tr_reads[i]}"
        ma = evs.merge_apsides(ap_reads[i])
        assert same([x[0] for x in ma], oat) and same([x[1] for x in ma], oad), f"{who}: merged {ma} vs {list(zip(oat, oad))}\nreads {ap_reads[i]}"
        assert [x[2] for x in ma] == oab.tolist() and [x[3] for x in ma] == oak.tolist(), f"{who}: merged {ma} vs {list(zip(oab, oak))}"
        if len(ott):
            last = tr_reads[i][-1][-1]
            assert bits(last[0]) == bits(ott[-1]) and last[1] == otb[-1], f"{who}: ends in {last}"
        for a, b in zip(tr_reads[i], tr_reads[i][1:]):
            searched_twice |= bool({x[0] for x in a[:-1]} & {x[0] for x in b})
    if name == "F-tr":
        assert searched_twice, f"{name} {method}: no step was searched twice: {tr_reads}"


@pytest.mark.parametrize("name,method", CASES)
def test_event_scene_on_the_wave_kernels(gpu, name, method):
    check_scene(gpu, name, method)


@pytest.mark.parametrize("name,method", T_CASES)
def test_thread_lane_scene_in_two_legs_and_on_a_clone(gpu, name, method):
    check_legs_and_clone(gpu, name, method)


@pytest.mark.parametrize("name,method", DRAIN_CASES)
def test_draining_a_slab_that_fills_inside_a_step(gpu, name, method):
    check_drained(gpu, name, method)


@pytest.mark.parametrize("form", ["thread-static", "thread-static-undealt", "thread-queue"])
def test_event_scenes_on_the_thread_forms(gpu, form):
    """every case above again on k_craft_events<false>, behind k_craft_propagate (craft dealt to the lanes, and craft i on lane i) and
    behind k_craft_queue"""
    env = dict(os.environ, EPH_CRAFT_FORM="thread", EPH_CRAFT_QUEUE="1" if form == "thread-queue" else "0",
               EPH_CRAFT_SORT="0" if form.endswith("undealt") else "2")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_gpu_craft_events.py"), form], env=env, cwd=str(ROOT), capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and f"{form} ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


# ---- the child: every case on the kernel form the environment selects -----------------------------------------------------------------
if __name__ == "__main__":
    import ephemeris_explorer_amd as ea
    assert os.environ.get("EPH_CRAFT_FORM") == "thread"
    try:
        for case in CASES:
            check_scene(ea, *case)
        for case in T_CASES:
            check_legs_and_clone(ea, *case)
        for case in DRAIN_CASES:
            check_drained(ea, *case)
    except AssertionError as e:                        # the head of the message names the case and the craft; the lists behind it are long
        print(f"{sys.argv[1]} FAILED: {str(e)[:1000]}")
        raise
    print(f"{sys.argv[1]} ok")
