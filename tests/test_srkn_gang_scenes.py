"""No GPU: the scenes of tests/srkn_gang_scenes.py on the C oracle alone -- the conditions they were planted for. What the device makes
of them is tests/test_gpu_srkn_gang.py."""
import numpy as np
import pytest

import gang_scenes as gs
import srkn_gang_scenes as sg
import srkn_scenes as ss
from conftest import load_system
from oracle import orc


@pytest.fixture(autouse=True)
def order_0():
    orc.set_pair_variant(0)
    yield
    orc.set_pair_variant(0)


def test_the_edge_gang_covers_what_it_names():
    gang = sg.edge_gang(0)
    assert [e.n for e in gang if not e.member.name.startswith("far")] == list(ss.SIZES)
    assert gang[sg.FAR_AT].member.name.startswith("far") and sg.FAR_AT != 0
    assert {ss.TABLES[e.table] for e in gang} == {(15, True), (4, False), (7, True), (3, False)}
    assert {np.sign(e.member.h) for e in gang} == {1.0, -1.0}
    assert sum(int((e.member.mu == 0.0).sum()) for e in gang) >= 1
    # an FSAL first stage both evaluated (no step taken yet) and carried (the carry of a launch before) inside one launch
    fsal_entries = {e.entry for e in gang if ss.TABLES[e.table][1]}
    assert 0 in fsal_entries and fsal_entries - {0}
    assert {e.entry for e in gang} == set(sg.ENTRY)


@pytest.mark.parametrize("variant", [0, 4])
def test_the_far_pair_is_outside_the_range_of_the_order_it_names(variant):
    E = gs.range_exponent(variant)
    e = sg.edge_gang(variant)[sg.FAR_AT]
    want = [gs.far_pair_index(False)]
    assert gs.out_of_range_pairs(e.member.pos, E) == want
    orc.set_pair_variant(variant)
    o = e.member.make(orc.NBody, e.table)
    assert o.advance(e.entry + sum(sg.EDGE_CALLS)) == 0
    pos, vel, _, _ = o.state()
    assert gs.out_of_range_pairs(pos, E) == want
    assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(o.acc()).all()
    if variant == 4:                                         # and inside the range of the orders below 4: the scene is that order's own
        assert gs.out_of_range_pairs(e.member.pos, gs.range_exponent(0)) == []


def test_every_bound_scene_stops_where_it_was_planted():
    members = sg.stop_members()
    assert sorted(m.steps for m in members) == [0, 0, 1, 3, sg.STOP_K, sg.STOP_K]
    assert [m.status for m in members].count(sg.STEP_SIZE_UNDERFLOW) == 1
    for m in members:
        o = m.make(orc.NBody)
        st = o.advance(sg.STOP_K)
        _, _, t, steps = o.state()
        assert (st, steps) == (m.status, m.steps), (m.name, st, steps)
        assert o.eval_count() == (ss.expected_evals(sg.STOP_TABLE, steps) if steps else 0), m.name
        if m.name == "exactly":                              # the bound fires on the step after the last: this call saw none of it
            assert t >= m.bound and o.advance(1) == sg.BOUND_REACHED
        if m.name == "underflow":
            assert t + m.member.h == t
    assert {name: sg.first_status(members, order) for name, order in sg.STOP_ORDERS.items()} == \
        {"underflow-first": sg.STEP_SIZE_UNDERFLOW, "bound-first": sg.BOUND_REACHED}
    for order in sg.STOP_ORDERS.values():
        assert sorted(order) == list(range(len(members)))


def test_the_clone_entries_are_distinct_states():
    m = sg.clone_source()
    seen = set()
    for entry in sg.CLONE_ENTRIES:
        o = m.make(orc.NBody, sg.CLONE_TABLE)
        assert o.advance(entry) == 0
        seen.add(o.state()[0].tobytes())
    assert len(seen) == len(sg.CLONE_ENTRIES) == 4


def test_the_convergence_scene_yields_at_least_three_rows():
    s = load_system(sg.SWEEP["system"])
    span = sg.SWEEP["days"] * 86400.0
    h, rows = orc.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + span, sg.SWEEP["method"], sg.SWEEP["h0"])
    assert len(s.mu) == 10 and len(rows) >= 3 and h == rows[-2][0] > 0.0
    assert len(rows) > 5                                     # more rows than one batch of candidates: a second batch follows
    assert sg.sweep_steps(rows, span, sg.SWEEP["h0"]) < sg.SWEEP_STEP_LIMIT // 4
