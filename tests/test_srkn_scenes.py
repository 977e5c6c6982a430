"""No GPU: the scenes of tests/srkn_scenes.py on the CPU oracles alone. The C oracle (orc.NBody(method=...), orc.Propagator(method=...))
is what tests/test_gpu_srkn_small.py compares the single-workgroup SRKN kernels with; here it is pinned, bit for bit, to the pure-Python
restatement of SRKN::advance (pyoracle.Srkn) on every scene and for all eight tables, and the conditions the scenes were planted for
are checked on it: the massless body moves, the far pair is outside the range of the wrapper-free sequences, an FSAL table evaluates
(stages - 1) * steps + 1 times and every other table stages * steps times."""
import copy

import numpy as np
import pytest

import gang_scenes as gs
import srkn_scenes as ss
from oracle import orc, pyoracle as po


class PyNBody:
    """pyoracle's Problem + Srkn behind the methods of orc.NBody"""

    def __init__(self, pos, vel, mu, t0, h, method):
        self.p, self.m, self.h = po.Problem(pos, vel, mu, t0), po.Srkn(method), float(h)

    def advance(self, k):
        for _ in range(k):
            st = self.m.advance(self.h, self.p)
            if st:
                return st
        return 0

    def state(self):
        return np.array(self.p.y, dtype=np.float64), np.array(self.p.dy, dtype=np.float64), self.p.time, self.m.i

    def acc(self):
        return np.array(self.m.ddy, dtype=np.float64)

    def eval_count(self):
        return self.p.evals

    def clone(self):
        c = copy.copy(self)                                   # Vec is immutable: new lists of the same elements are a deep copy
        c.p, c.m = copy.copy(self.p), copy.copy(self.m)
        c.p.y, c.p.dy = list(self.p.y), list(self.p.dy)
        c.m.ddy = None if self.m.ddy is None else list(self.m.ddy)
        return c


@pytest.fixture(scope="module")
def oracle():
    orc.set_pair_variant(0)
    return ss.Oracle()


def test_the_tables_are_the_reference_s_eight():
    assert sorted(ss.TABLES) == sorted(["BlanesMoan6B", "BlanesMoan11B", "BlanesMoan14A", "ForestRuth", "McLachlanO4", "McLachlanSS17",
                                        "Pefrl", "Ruth"])
    for table, (stages, fsal) in ss.TABLES.items():
        a, b, f = orc.srkn_coeffs(table)
        assert (len(a), len(b), bool(f)) == (stages, stages, fsal), table
        assert stages <= 32                                  # the bound of SrknCoeffs: what the kernel's arguments hold
    assert ss.TABLES[ss.FSAL_TABLE][1] and not ss.TABLES[ss.PLAIN_TABLE][1]
    assert sum(k for op, k in ss.OPS if op != "clone") == ss.TOTAL_STEPS


def test_the_sizes_cross_every_threshold_of_the_frame():
    sizes = set(ss.SIZES)
    assert {1, 2, 3, 31, 32} <= sizes
    for lo, hi in ((10, 11), (21, 22)):                      # the chain threads spill into the next wave
        assert {lo, hi} <= sizes and gs.owner_waves(lo) + 1 == gs.owner_waves(hi)
    assert {16, 17} <= sizes and gs.row_length(16) == 16 and gs.row_length(17) == 32
    ms = ss.members()
    assert {m.n for m in ms} == sizes
    assert {np.sign(m.h) for m in ms} == {1.0, -1.0}
    assert any((m.mu == 0.0).sum() == 1 for m in ms) and all(len(set(m.mu)) == m.n for m in ms)


@pytest.mark.parametrize("table", list(ss.TABLES))
def test_the_c_oracle_equals_the_python_restatement(oracle, table):
    po.set_pair_variant(0)
    for m in ss.members() + ss.far_members(0):
        ss.compare(oracle.records(m, table), ss.run(m, table, PyNBody), f"{table}, {m.name}: orc.NBody against pyoracle.Srkn")


@pytest.mark.parametrize("table", list(ss.TABLES))
def test_evaluation_counts_and_the_massless_body(oracle, table):
    for m in ss.members():
        recs = oracle.records(m, table)
        steps = [1, 6, 6, 6, 7, 6, 18, 17]                  # after every operation; from the clone on: handle, clone
        assert [int(r["steps"][0]) for r in recs] == steps, (table, m.name)
        assert [int(r["evals"][0]) for r in recs] == [ss.expected_evals(table, s) for s in steps], (table, m.name)
        assert all(np.isfinite(r[k]).all() for r in recs for k in ("pos", "vel", "acc")), (table, m.name)
        if m.n == 1:
            assert all(np.array_equal(gs.bits(r["acc"]), np.zeros((1, 3), dtype=np.uint64)) for r in recs)      # +0.0
        massless = np.flatnonzero(m.mu == 0.0)
        if len(massless) and m.n > 1:
            b = int(massless[0])
            assert np.abs(recs[-1]["acc"][b]).max() > 0.0 and not np.array_equal(recs[-1]["pos"][b], m.pos[b]), (table, m.name)


@pytest.mark.parametrize("variant", [0, 4])
def test_the_far_pair_is_out_of_range_for_the_orders_tested(variant):
    E = gs.range_exponent(variant)
    orc.set_pair_variant(variant)
    try:
        for mirrored, m in enumerate(ss.far_members(variant)):
            want = [gs.far_pair_index(bool(mirrored))]
            for table in (ss.FSAL_TABLE, ss.PLAIN_TABLE):
                o = m.make(orc.NBody, table)
                assert gs.out_of_range_pairs(m.pos, E) == want
                for _ in range(ss.TOTAL_STEPS):
                    assert o.advance(1) == 0
                pos, vel, _, _ = o.state()
                assert gs.out_of_range_pairs(pos, E) == want, (table, m.name)
                assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(o.acc()).all()
    finally:
        orc.set_pair_variant(0)


class PySrknPropagator(po.Propagator):
    """pyoracle.Propagator's solout around pyoracle.Srkn (the restatement's own constructor knows the multistep methods only)"""

    class _Integ:
        def __init__(self, method, h, p):
            self.m, self.h, self.p = po.Srkn(method), h, p

        def advance(self):
            return self.m.advance(self.h, self.p)

    def __init__(self, pos, vel, mu, t0, dt, direction, count, degree, method):
        self.p = po.Problem(pos, vel, mu, t0)
        self.dir = 1 if direction > 0 else -1
        self.dt = dt
        self.integ = self._Integ(method, abs(dt) * self.dir, self.p)
        self.period = [dt * float(c) for c in count]
        self.degree = list(degree)
        self.last = [0.0] * len(mu)
        self.window = [[self.p.y[b]] for b in range(len(mu))]
        self.taus = [i / 8.0 if self.dir > 0 else 1.0 - i / 8.0 for i in range(9)]
        self.solution = self._new_solution()


@pytest.mark.parametrize("table", ss.SAMPLED_TABLES)
def test_the_c_propagator_equals_the_python_restatement(table):
    """the restatement has no step_to and no clone: both are stepped 6 and then 100 times, with a take after each"""
    po.set_pair_variant(0)
    orc.set_pair_variant(0)
    for m in ss.sampled_members():
        a, b = m.make(orc.Propagator, table), m.make(PySrknPropagator, table)
        for steps in (6, 100):
            for _ in range(steps):
                assert a.step() == 0 and b.step() == 0
            sa, sb = a.take_solution(), b.take_solution()
            for body in range(m.n):
                co, nc = sa.coeffs(body)
                assert sa.info(body) == (sb[body]["start"], sb[body]["interval"], len(sb[body]["polys"])), (table, m.name, steps, body)
                for q, poly in enumerate(sb[body]["polys"]):
                    want = np.zeros((8, 3))
                    want[:len(poly)] = [[float(x) for x in v] for v in poly]
                    assert nc[q] == len(poly) and np.array_equal(gs.bits(co[q]), gs.bits(want)), (table, m.name, steps, body, q)
        pos, vel, t, c = a.state()
        assert (t, c) == (b.p.time, 106)
        assert np.array_equal(gs.bits(pos), gs.bits(np.array(b.p.y, dtype=np.float64)))
        assert np.array_equal(gs.bits(vel), gs.bits(np.array(b.p.dy, dtype=np.float64)))


@pytest.mark.parametrize("table", ss.SAMPLED_TABLES)
def test_sampled_scenes_are_live_on_the_c_oracle(table):
    """the propagator scenes reach what they are for: the take six steps in finds every window partly filled (nine samples make one), at the end every body has polynomials; the clone continues as the original"""
    for m in ss.sampled_members():
        out = dict(ss.run_sampled(m, table, orc.Propagator))
        early, last, twin = out["take at 6 steps"], out["final take and state, original"], out["final take and state, clone"]
        assert (early["npoly"] == 0).all(), (table, m.name, early["npoly"])      # six steps: every window is partly filled
        assert (last["npoly"] > 0).all(), (table, m.name, last["npoly"])
        assert np.isfinite(last["coef"]).all()
        ss.compare_sampled([("x", last)], [("x", twin)], f"{table}, {m.name}: clone against original")
        assert int(last["steps"][0]) >= 100
