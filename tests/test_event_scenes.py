"""CPU: the scenes of tests/event_scenes.py on the two restatements of the reference's SpacecraftSolout -- orc.Craft (C) against
pyoracle.Craft (Python) on the same parts -- bit for bit: knots, SOI transitions and apsides; and every scene's liveness predicate (a
scene that stops stepping on what it was planted for fails here, without a GPU). The C / Python pair is the arbiter of
tests/test_gpu_craft_events.py, which runs the same scenes on the device."""
import numpy as np
import pytest

import event_scenes as evs
import synthetic_tables as syn
from craft_cases import bits, same
from oracle import orc, pyoracle as po

SCENES = {sc.name: sc for sc in evs.scenes() + evs.drain_scenes()}
CASES = [(name, m) for name, sc in SCENES.items() for m in sc.methods]


@pytest.fixture(scope="module")
def solutions():
    return {name: (orc.Solution.from_parts(*sc.table), syn.python_table(sc.table)) for name, sc in SCENES.items()}


def test_a_body_at_rest_needs_two_rows(solutions):
    """what the tables rest on: [p, 0] evaluates to p with velocity 0 over the whole span, in both restatements"""
    sc = SCENES["N"]
    sol, table = solutions["N"]
    for b in range(sc.n_bodies):
        for t in (0.0, 64.0, 8192.0, evs.SPAN):
            p, v = sol.eval(b, t)
            q = po.spline_eval(table[b]["start"], table[b]["interval"], table[b]["polys"], t)
            assert same(p, sc.points[b]) and not v.any() and same(q[0], p) and same(q[1], v), (b, t, p, v)


@pytest.mark.parametrize("name,method", CASES)
def test_scene_is_live_and_the_restatements_agree(solutions, name, method):
    """the liveness predicate on the C oracle's lists, then status, every knot, every transition and every apsis of the craft in
    sc.py_craft against the Python restatement (both on this host's libm pow: pyoracle calls math.pow)"""
    sc = SCENES[name]
    sol, table = solutions[name]
    orc.set_pow_mode(1)
    try:
        res = evs.run_oracle(sc, method, sol)
        sc.liveness(sc, method, res)
        for i in sc.py_craft:
            st, p = evs.run_python(sc, method, i, table)
            c = res[i]["craft"]
            assert st == res[i]["status"], (name, method, i, st, res[i]["status"])
            kt, kp, kv = c.knots()
            assert len(kt) == len(p.knots), (name, method, i)
            assert same(kt, [k[0] for k in p.knots]) and same(kp, [k[1][:3] for k in p.knots]) and same(kv, [k[1][3:] for k in p.knots]), \
                (name, method, i)
            tt, tb = c.transitions()
            assert len(tt) == len(p.transitions) and same(tt, [x[0] for x in p.transitions]) and list(tb) == [x[1] for x in p.transitions], \
                (name, method, i, tt, tb, p.transitions)
            at, ad, ab, ak = c.apsides()
            assert len(at) == len(p.apsides) and same(at, [x[0] for x in p.apsides]) and same(ad, [x[1] for x in p.apsides]), \
                (name, method, i, at, p.apsides)
            assert list(ab) == [x[2] for x in p.apsides] and list(ak) == [x[3] for x in p.apsides], (name, method, i)
    finally:
        orc.set_pow_mode(0)
    # and the pinned pow: the liveness holds for the results the device is compared with as well
    sc.liveness(sc, method, evs.run_oracle(sc, method, sol))


def test_merging_drained_lists_restates_insert():
    """merge_transitions / merge_apsides (what tests/test_gpu_craft_events.py does with the lists of a drained batch): a list read twice, an
    entry in front of what was read before and an entry the same-body rule drops all merge to the one history"""
    whole = [(0.0, 0), (10.0, 3), (20.0, 2), (30.0, 1), (40.0, 3)]
    reads = [whole[:1], [(0.0, 0), (20.0, 2), (30.0, 1)], [(10.0, 3), (20.0, 2), (30.0, 1)], [(30.0, 1), (40.0, 3), (45.0, 3)]]
    assert evs.merge_transitions(reads) == whole
    aps = [(1.0, 5.0, 0, 0), (2.0, 6.0, 1, 1), (3.0, 7.0, 0, 0)]
    assert evs.merge_apsides([aps[1:2], aps[:2], aps[2:], aps[1:]]) == aps
    assert np.array_equal(bits([a[1] for a in evs.merge_apsides([[(1.0, 5.0, 0, 0)], [(1.0, -0.0, 0, 0)]])]), bits([-0.0]))   # equal time: overwrite
