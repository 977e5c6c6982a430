"""CPU: the scenarios of tests/synthetic_tables.py on the two restatements of the reference -- orc.Craft over orc.Solution.from_parts (C)
against pyoracle.Craft over the same parts (Python) -- bit for bit, every scenario's liveness predicate (a scenario that stops stepping on
its planted epochs fails here, without a GPU), and the two direct evaluators at the planted epochs. The C / Python pair is the arbiter of
tests/test_gpu_craft_lookup.py, which runs the same scenarios on the device."""
import numpy as np
import pytest

import synthetic_tables as syn
from craft_cases import bits, same
from oracle import orc, pyoracle as po

SCENARIOS = {sc.name: sc for sc in syn.scenarios()}
CASES = [(name, m) for name, sc in SCENARIOS.items() for m in sc.methods]


def test_from_parts_copies_ncoef_rows_and_keeps_signed_zeros(product_lib):
    """orc.Solution.from_parts and the product's Solution.from_parts give back what they were given, bit for bit (-0.0 included), zero
    padded behind ncoef; orc_solution_create takes ncoef rows per polynomial and nothing behind them (rows poisoned with NaN)."""
    ea = product_lib
    sc = SCENARIOS["D-huge-middle"]
    so, sp = orc.Solution.from_parts(*sc.table), ea.Solution.from_parts(*sc.table)
    zeros = 0
    for b, (start, interval, polys) in enumerate(zip(*sc.table)):
        assert so.info(b) == sp.info(b) == (start, interval, len(polys))
        for co, nc in (so.coeffs(b), sp.coeffs(b)):
            assert list(nc) == [len(p) for p in polys]
            for p, rows in enumerate(polys):
                assert same(co[p, :len(rows)], rows) and not bits(co[p, len(rows):]).any(), (b, p)
                zeros += int(np.count_nonzero(bits(rows) == bits(-0.0)))
    assert zeros > 20 and any(len(p) == 0 for p in sc.table[2][2]) and {len(p) for body in sc.table[2] for p in body} == set(range(9))
    # poison: every row at or beyond ncoef is NaN in the caller's buffer
    L = orc.lib()
    npoly = np.array([len(p) for p in sc.table[2]], dtype=np.int64)
    co, nc = np.full((int(npoly.sum()), 8, 3), np.nan), np.zeros(int(npoly.sum()), dtype=np.int32)
    flat = [rows for body in sc.table[2] for rows in body]
    for q, rows in enumerate(flat):
        co[q, :len(rows)], nc[q] = rows, len(rows)
    import ctypes as C
    h = L.orc_solution_create(len(npoly), orc._ptr(orc._f64(sc.table[0])), orc._ptr(orc._f64(sc.table[1])),
                              orc._ptr(npoly, C.POINTER(C.c_int64)), orc._ptr(co), orc._ptr(nc, orc._i32p))
    poisoned = orc.Solution(L, h)
    for b in range(sc.n_bodies):
        assert same(poisoned.coeffs(b)[0], so.coeffs(b)[0])
        for t in syn.planted_epochs(sc, b):
            r, w = poisoned.eval(b, t), so.eval(b, t)
            assert (r is None) == (w is None) and (r is None or (same(r[0], w[0]) and same(r[1], w[1])))
    with pytest.raises(ValueError):
        orc.Solution.from_parts([0.0], [1.0], [[np.zeros((9, 3))]])


@pytest.fixture(scope="module")
def solutions():
    return {name: (orc.Solution.from_parts(*sc.table), syn.python_table(sc.table)) for name, sc in SCENARIOS.items()}


@pytest.mark.parametrize("name,method", CASES)
def test_scenario_is_live_and_the_restatements_agree(solutions, name, method):
    """the liveness predicate on the C oracle's results for every craft, then status, attempts, time, state, next_h and every knot of
    the craft in sc.py_craft against the Python restatement (both on this host's libm pow: pyoracle calls math.pow)"""
    sc = SCENARIOS[name]
    sol, table = solutions[name]
    variants = (0, 4) if name == "A" and method == "Verner87" else (0,)
    for variant in variants:
        orc.set_pow_mode(1)
        orc.set_pair_variant(variant)
        po.set_pair_variant(variant)
        try:
            res = syn.run_oracle(sc, method, sol)
            sc.liveness(sc, method, res)
            for i in sc.py_craft:
                st, p = syn.run_python(sc, method, i, table)
                c = res[i]["craft"]
                cs = c.state()
                assert st == res[i]["status"], (name, method, i, st, res[i]["status"])
                assert cs["attempts"] == p.n and bits(cs["next_h"]) == bits(p.next_h) and bits(cs["t"]) == bits(p.t), (name, method, i)
                assert same(cs["pos"], p.y[:3]) and same(cs["vel"], p.y[3:]), (name, method, i)
                kt, kp, kv = c.knots()
                assert len(kt) == len(p.knots), (name, method, i)
                assert same(kt, [k[0] for k in p.knots]) and same(kp, [k[1][:3] for k in p.knots]) and same(kv, [k[1][3:] for k in p.knots]), \
                    (name, method, i)
        finally:
            orc.set_pow_mode(0)
            orc.set_pair_variant(0)
            po.set_pair_variant(0)
    # and the pinned pow: the liveness holds for the results the device is compared with as well
    sc.liveness(sc, method, syn.run_oracle(sc, method, sol))


@pytest.mark.parametrize("name", ["A", "B-inexact", "C", "D-huge-middle", "D-65"])
def test_evaluators_at_the_planted_epochs(solutions, name):
    """orc.Solution.eval (UniformSpline::position and ::state_vector) against pyoracle.spline_position / spline_eval at start, every
    boundary and its two neighbours, start + span and its upper neighbour, +-inf"""
    sc = SCENARIOS[name]
    sol, table = solutions[name]
    inside = 0
    for b in range(sc.n_bodies):
        e = table[b]
        for t in syn.planted_epochs(sc, b):
            t = float(t)
            want = po.spline_eval(e["start"], e["interval"], e["polys"], t)
            wpos = po.spline_position(e["start"], e["interval"], e["polys"], t)
            got, gpos = sol.eval(b, t), sol.eval(b, t, with_velocity=False)
            assert (want is None) == (got is None) == (wpos is None) == (gpos is None), (name, b, t)
            if want is not None:
                inside += 1
                assert same(got[0], want[0]) and same(got[1], want[1]) and same(gpos, wpos), (name, b, t)
        s, iv, n = sc.table[0][b], sc.table[1][b], len(sc.table[2][b])
        end = s + iv * float(n)                                       # (rounds where the table starts at 2^60)
        assert sol.eval(b, s) is not None and (sol.eval(b, end) is not None) == (end - s <= iv * float(n))       # both ends are inside
        assert sol.eval(b, np.nextafter(s, -np.inf)) is None and sol.eval(b, np.inf) is None and sol.eval(b, -np.inf) is None
    assert inside > 3 * sc.n_bodies
