"""-m gpu: k_srkn_small / k_srkn_double_small (csrc/step_srkn_small.hip) -- a symplectic Runge-Kutta-Nystrom handle of at most 32
bodies advances in ONE launch per advance() -- against the C oracle (pinned to the Python restatement by tests/test_srkn_scenes.py)
and against the per-stage launches (set_path(1)), the second witness. Every comparison is on bit patterns (view(np.uint64)): no
tolerance appears anywhere.

On the commit before these kernels every bit comparison below already passes, there through per-stage launches (one launch per
stage, two on a `<Double>` handle): the scenes test the kernels, not a change of meaning. What fails there is the launch count:
test_advance_is_one_launch, and the last line of test_one_year_of_the_shipped_system_in_one_launch."""
import numpy as np
import pytest

import gang_scenes as gs
import srkn_scenes as ss
from conftest import load_system
from oracle import orc

pytestmark = pytest.mark.gpu

YEAR = 365 * 86400.0
INF = float("inf")
bits = gs.bits


class Order:
    """evaluation order k of the point-mass term for the product's new handles and for the C oracle, while the block runs"""

    def __init__(self, gpu, k):
        self.gpu, self.k = gpu, k

    def __enter__(self):
        self.before = self.gpu.pair_variant()
        self.gpu.set_pair_variant(self.k)
        orc.set_pair_variant(self.k)

    def __exit__(self, *exc):
        self.gpu.set_pair_variant(self.before)
        orc.set_pair_variant(0)


_oracles = {}


def oracle_of(order):
    """the oracle's runs in evaluation order `order`, shared by the tests of this module (call inside Order(gpu, order))"""
    return _oracles.setdefault(order, ss.Oracle())


def check_scene(gpu, m, table, order):
    want = oracle_of(order).records(m, table)
    label = f"{table}, {m.name}, order {order}"
    got = ss.run(m, table, gpu.NBodyIntegration)
    ss.compare(got, want, f"{label}: one launch against the oracle")
    per_stage = ss.run(m, table, gpu.NBodyIntegration, prepare=lambda h: h.set_path(1))
    ss.compare(per_stage, got, f"{label}: per-stage launches against one launch")


# ---- 1. plain scenes
@pytest.mark.parametrize("table", list(ss.TABLES))
def test_every_scene_under_every_table(gpu, table):
    with Order(gpu, 0):
        for m in ss.members() + ss.far_members(0):
            check_scene(gpu, m, table, 0)


@pytest.mark.parametrize("table", [ss.FSAL_TABLE, ss.PLAIN_TABLE])
def test_every_scene_at_order_4(gpu, table):
    """orders 4-6 leave the wrapper-free sequences at a squared distance of 2^133: the far pair sits there"""
    with Order(gpu, 4):
        for m in ss.members() + ss.far_members(4):
            check_scene(gpu, m, table, 4)


@pytest.mark.parametrize("order", range(7))
def test_all_seven_orders_at_17_bodies(gpu, order):
    with Order(gpu, order):
        for table in (ss.FSAL_TABLE, ss.PLAIN_TABLE):
            check_scene(gpu, gs.edge_member(17, 1), table, order)


# ---- 2. one launch (the test that fails without the kernels: the symplectic branch opened no timing interval and counted nothing)
@pytest.fixture(scope="module")
def full():
    return load_system("full_solar_system_2433282.5")


def test_advance_is_one_launch(gpu, full):
    s = full
    g = gpu.NBodyIntegration(s.pos, s.vel, s.mu, s.epoch, s.dt, "BlanesMoan14A")
    g.enable_timing()
    launches = g.kernel_time()[1]
    for k in (1, 23):
        g.advance(k)
        ms, now = g.kernel_time()
        assert now == launches + 1, (k, now, launches)
        launches = now
    assert ms > 0.0
    o = orc.NBody(s.pos, s.vel, s.mu, s.epoch, s.dt, "BlanesMoan14A")
    assert o.advance(24) == 0
    assert ss.same_record(ss.record(g), ss.record(o)) is None


# ---- 3. bound
def test_bound_reached_inside_a_launch(gpu):
    m = gs.edge_member(32, 1)
    bound = m.t0 + 30.5 * m.h
    g, o = m.make(gpu.NBodyIntegration, "Pefrl"), m.make(orc.NBody, "Pefrl")
    g.set_bound(bound)
    o.set_bound(bound)
    with pytest.raises(gpu.StepError) as e:
        g.advance(100)
    assert e.value.status == gpu.BOUND_REACHED and o.advance(100) == gpu.BOUND_REACHED
    rec = ss.record(g)
    assert int(rec["steps"][0]) == 31 and rec["t"][0] > bound
    ss.compare([rec], [ss.record(o)], "Pefrl, 31 steps to the bound")
    g.set_bound(INF)
    o.set_bound(INF)
    twin = g.clone()
    for h in (g, twin):
        h.advance(7)
    assert o.advance(7) == 0
    ss.compare([ss.record(g), ss.record(twin)], [ss.record(o)] * 2, "Pefrl, 7 steps behind the lifted bound, handle and clone")


# ---- 4. compensated
def oracle_after(pos, vel, mu, h, method, k):
    st, y, dy, end = orc.double_solve(pos, vel, mu, 0.0, INF, h, method, max_steps=k)
    assert st == 0
    return y[..., 0], dy[..., 0], end


def assert_state(g, want, count, what):
    p, v, t, c = g.state()
    assert c == count and t == want[2], (what, c, t, want[2])
    assert np.array_equal(bits(p), bits(want[0])), (what, "positions", int((bits(p) != bits(want[0])).sum()))
    assert np.array_equal(bits(v), bits(want[1])), (what, "velocities", int((bits(v) != bits(want[1])).sum()))


@pytest.mark.parametrize("method", ["BlanesMoan14A", "BlanesMoan6B", "Ruth"])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 22, 32])
def test_compensated_handles(gpu, n, method):
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    h = 1.0 / 1024.0
    a = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, method + "<Double>")
    b = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, method + "<Double>")
    plain = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, method)          # created beside the tagged ones: its usual bits
    assert a.compensated and b.compensated and not plain.compensated
    b.set_path(1)
    twins, done = None, 0
    for op, k in (("advance", 1), ("advance", 7), ("clone", 0), ("advance", 1), ("advance_both", 9)):
        if op == "clone":
            twins = (a.clone(), b.clone())
            continue
        a.advance(k)
        b.advance(k)
        done += k
        want = oracle_after(pos, vel, mu, h, method, done)
        assert_state(a, want, done, (n, method, done, "one launch"))
        assert_state(b, want, done, (n, method, done, "per-stage launches"))
        assert np.array_equal(bits(a.acc()), bits(b.acc())), (n, method, done)
        assert a.eval_count() == b.eval_count() == ss.expected_evals(method, done), (n, method, done)
        if op == "advance_both":
            for c in twins:
                c.advance(k)
                assert_state(c, oracle_after(pos, vel, mu, h, method, done - 1), done - 1, (n, method, "clone"))
            assert np.array_equal(bits(twins[0].acc()), bits(twins[1].acc())), (n, method, "clones")
    plain.advance(done)
    o = orc.NBody(pos, vel, mu, 0.0, h, method)
    assert o.advance(done) == 0
    assert ss.same_record(ss.record(plain), ss.record(o)) is None, (n, method, "the plain neighbour")
    if n > 1:                                                            # (one body: no force, and both forms add the same products)
        assert not np.array_equal(bits(plain.state()[0]), bits(a.state()[0]))   # the compensation was live


# ---- 5. a year in one launch
def test_one_year_of_the_shipped_system_in_one_launch(gpu, full):
    """32 bodies, BlanesMoan14A<Double>, h = 1200 s, bound = epoch + 365 d: 26 280 steps (31 536 000 / 1200, exact) of 15 stages in
    one advance, which ends as the reference's solve does (BoundReached on the step after the last). The oracle's side takes about
    3 s on one core."""
    s = full
    bound = s.epoch + YEAR
    g = gpu.NBodyIntegration(s.pos, s.vel, s.mu, s.epoch, 1200.0, "BlanesMoan14A<Double>")
    g.set_bound(bound)
    g.enable_timing()
    with pytest.raises(gpu.StepError) as e:
        g.advance(1 << 40)
    assert e.value.status == gpu.BOUND_REACHED
    st, y, dy, end = orc.double_solve(s.pos, s.vel, s.mu, s.epoch, bound, 1200.0, "BlanesMoan14A", native=True)
    assert st == 0 and end == bound
    assert_state(g, (y[..., 0], dy[..., 0], end), 26280, "one year")
    assert g.kernel_time()[1] == 1


# ---- 6. sampled
@pytest.mark.parametrize("table", ss.SAMPLED_TABLES)
def test_sampled_scenes(gpu, table):
    with Order(gpu, 0):
        for m in ss.sampled_members():
            want = ss.run_sampled(m, table, orc.Propagator)
            got = ss.run_sampled(m, table, lambda *a: gpu.NBodyPropagator(*a[:8], method=a[8]))
            ss.compare_sampled(got, want, f"{table}, {m.name}")


# ---- 7. a symplectic member of an advance_many
def test_advance_many_with_a_symplectic_member(gpu, full):
    s = full
    args = (s.pos, s.vel, s.mu, s.epoch, s.dt)
    methods = ("QuinlanTremaine12", "BlanesMoan6B", "QuinlanTremaine12")
    gang = [gpu.NBodyIntegration(*args, m) for m in methods]
    alone = [gpu.NBodyIntegration(*args, m) for m in methods]
    for k in (12, 9):
        gpu.advance_many(gang, k)
        for h in alone:
            h.advance(k)
        for m, g, h in zip(methods, gang, alone):
            assert ss.same_record(ss.record(g), ss.record(h)) is None, (m, k)
    o = orc.NBody(*args, "BlanesMoan6B")
    assert o.advance(21) == 0
    assert ss.same_record(ss.record(gang[1]), ss.record(o)) is None


# ---- 8. what did not change
@pytest.mark.parametrize("n", [33, 65])
def test_more_than_32_bodies_keep_the_per_stage_launches(gpu, n):
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    h = 1.0 / 1024.0
    o = orc.NBody(pos, vel, mu, 0.0, h, "BlanesMoan6B")
    want = {}
    for k, step in ((1, 1), (6, 5)):
        assert o.advance(step) == 0
        want[k] = (ss.record(o), oracle_after(pos, vel, mu, h, "BlanesMoan6B", k))
    for path in (0, 1, 2) if n == 33 else (0, 1):
        g = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, "BlanesMoan6B")
        d = gpu.NBodyIntegration(pos, vel, mu, 0.0, h, "BlanesMoan6B<Double>")
        for x in (g, d):
            x.set_path(path)
            x.enable_timing()
        for k, step in ((1, 1), (6, 5)):
            g.advance(step)
            d.advance(step)
            assert ss.same_record(ss.record(g), want[k][0]) is None, (n, path, k)
            assert_state(d, want[k][1], k, (n, path, k, "<Double>"))
            assert d.eval_count() == ss.expected_evals("BlanesMoan6B", k)
        assert g.kernel_time()[1] == 0 and d.kernel_time()[1] == 0      # (the per-stage launches are not counted, as before)
