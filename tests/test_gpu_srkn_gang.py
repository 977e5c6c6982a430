"""-m gpu: the symplectic members of eph_nbody_advance_many / eph_prop_step_n_many in one launch (k_srkn_small_many<SrknPlain> /
<SrknDouble>, csrc/step_srkn_small.hip: a workgroup per system, every member with its own step count), and convergence_gang(), the
caller that steps the runs of a convergence sweep side by side. Scenes: tests/srkn_gang_scenes.py.

Every comparison is on bit patterns: against orc.NBody / orc.Propagator / the oracle's Double solver, and against a twin handle
advanced alone (one launch of k_srkn_small / k_srkn_double_small). No tolerance appears anywhere.

On the commit before the gang kernels every bit comparison here passes already -- a symplectic member of advance_many was advanced
on its own. What fails there is the launch count: test_launch_counts, the probes of the other tests, and convergence_gang itself.
Launches are read as tests/test_gpu_startup_small.py reads them: through eph_debug_wg_cycles of the test-hooks library (a shared
launch counts once), and through gang_scenes.LaunchProbe on the product (a member that is not the lead counts the shared launch and
gains no milliseconds of its own)."""
import ctypes as C

import numpy as np
import pytest

import gang_scenes as gs
import srkn_gang_scenes as sg
import srkn_scenes as ss
from conftest import load_system
from hooks import failing_allocations
from oracle import orc
from test_gpu_srkn_small import Order
from test_gpu_startup_small import Counted

pytestmark = pytest.mark.gpu

INF = float("inf")
bits = gs.bits
KINDS = pytest.mark.parametrize("compensated", [False, True], ids=["plain", "double"])


# ---- the oracle's side, computed once per key and left unchanged
_plain, _double = {}, {}


def oracle_record(order, member, table, steps):
    """ss.record of orc.NBody after `steps` steps from the start, in evaluation order `order` (call inside Order(gpu, order))"""
    key = (order, member.name, table)
    if key not in _plain:
        _plain[key] = (member.make(orc.NBody, table), [])
        _plain[key][1].append(ss.record(_plain[key][0]))
    o, trail = _plain[key]
    while len(trail) <= steps:
        assert o.advance(1) == 0, key
        trail.append(ss.record(o))
    return trail[steps]


def double_record(order, member, table, steps):
    """value parts, time, step count and evaluation count of the oracle's Double solver after `steps` steps"""
    key = (order, member.name, table, steps)
    if key not in _double:
        if steps:
            st, y, dy, end = orc.double_solve(member.pos, member.vel, member.mu, member.t0, INF, member.h, table, max_steps=steps)
            assert st == 0, key
            pos, vel = y[..., 0].copy(), dy[..., 0].copy()
        else:
            pos, vel, end = np.array(member.pos, dtype=np.float64), np.array(member.vel, dtype=np.float64), member.t0
        _double[key] = dict(pos=pos, vel=vel, t=np.array([end]), steps=np.array([steps], dtype=np.int64),
                            evals=np.array([ss.expected_evals(table, steps) if steps else 0], dtype=np.int64))
    return _double[key]


def assert_record(got, want, where, keys=("t", "steps", "evals", "pos", "vel", "acc")):
    for key in keys:
        g, w = got[key], want[key]
        assert g.shape == w.shape, f"{where}: {key}: {g.shape} against {w.shape}"
        if np.array_equal(bits(g), bits(w)):
            continue
        if g.ndim < 2:
            raise AssertionError(f"{where}: {key} {g!r} against {w!r}")
        bad = np.flatnonzero((bits(g) != bits(w)).any(axis=1))
        raise AssertionError(f"{where}: {key} of body {int(bad[0])} ({len(bad)} of {len(g)} bodies differ): {g[int(bad[0])]} against {w[int(bad[0])]}")


def assert_against_oracle(rec, order, compensated, member, table, steps, where):
    if compensated:
        assert_record(rec, double_record(order, member, table, steps), f"{where}: against the oracle's Double solver",
                      keys=("t", "steps", "evals", "pos", "vel"))
    else:
        assert_record(rec, oracle_record(order, member, table, steps), f"{where}: against orc.NBody")


def status_of(call):
    """the StepError status of call(), 0 where it returns"""
    import ephemeris_explorer_amd as ea
    try:
        call()
    except ea.StepError as e:
        return e.status
    return 0


# ---- 1. edges
@KINDS
@pytest.mark.parametrize("order", [0, 4])
def test_edges(gpu, order, compensated):
    """one member per size, tables of 15, 4, 7 and 3 stages by turns, both signs, a massless body, entered after 0, 1 or 5 steps;
    the far pair in a workgroup other than 0. After every call: against the oracle and against a twin advanced alone"""
    with Order(gpu, order):
        scene = sg.edge_gang(order)
        gang, alone = ([e.member.make(gpu.NBodyIntegration, e.table, compensated=compensated) for e in scene] for _ in range(2))
        for e, g, a in zip(scene, gang, alone):
            if e.entry:
                g.advance(e.entry)
                a.advance(e.entry)
        probe = gs.LaunchProbe(gang[sg.FAR_AT])
        for k, done in zip(sg.EDGE_CALLS, sg.edge_steps()):
            gpu.advance_many(gang, k)
            probe.assert_ganged(f"order {order}: advance_many({k}), the far member")
            for e, g, a in zip(scene, gang, alone):
                where = f"order {order}, {'<Double>' if compensated else 'plain'}: {e.name} after advance_many({k})"
                a.advance(k)
                rec = ss.record(g)
                assert_record(rec, ss.record(a), f"{where}: against the twin advanced alone")
                assert_against_oracle(rec, order, compensated, e.member, e.table, e.entry + int(done), where)


# ---- 2. launch counts: what fails without the gang kernels
class CountedGang(Counted):
    def __init__(self, hooks):
        super().__init__(hooks)
        dp = C.POINTER(C.c_double)
        self.L.eph_nbody_get_acc.argtypes = [C.c_void_p, dp]
        self.L.eph_nbody_eval_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self.L.eph_last_error.restype = C.c_char_p

    def make(self, member, table, compensated=False):
        return self.fresh(member, table, compensated)

    def record(self, h, n):
        pos, vel, acc = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        dp, t, c, e = C.POINTER(C.c_double), C.c_double(), C.c_uint32(), C.c_uint64()
        assert self.L.eph_nbody_get_state(h, pos.ctypes.data_as(dp), vel.ctypes.data_as(dp), C.byref(t), C.byref(c)) == 0
        assert self.L.eph_nbody_get_acc(h, acc.ctypes.data_as(dp)) == 0 and self.L.eph_nbody_eval_count(h, C.byref(e)) == 0
        return dict(pos=pos, vel=vel, acc=acc, t=np.array([t.value]), steps=np.array([c.value], dtype=np.int64),
                    evals=np.array([e.value], dtype=np.int64))


@pytest.fixture
def counted(hooks):
    c = CountedGang(hooks)
    yield c
    c.close()


def test_launch_counts(counted):
    """three plain symplectic members: ONE launch (three before the gang); three plain and three <Double>: two; two and a member of
    33 bodies: one, and the big one's own; a group of one keeps its own advance"""
    a, b, c = gs.edge_member(32, 1), gs.edge_member(17, -1), gs.edge_member(3, 1)
    gang = [counted.make(a, "BlanesMoan14A"), counted.make(b, "McLachlanO4"), counted.make(c, "Ruth")]
    assert counted.advance_many(gang, 9) == 1 and [counted.steps(h) for h in gang] == [9] * 3
    assert counted.advance_many(gang, 4) == 1 and [counted.steps(h) for h in gang] == [13] * 3
    mixed = [counted.make(a, "BlanesMoan6B"), counted.make(a, "BlanesMoan6B", True), counted.make(b, "Ruth", True),
             counted.make(b, "Pefrl"), counted.make(c, "BlanesMoan14A", True), counted.make(c, "BlanesMoan14A")]
    assert counted.advance_many(mixed, 6) == 2 and [counted.steps(h) for h in mixed] == [6] * 6
    big = gs.Member("n33", *gs.random_system(33), gs.H)
    own = counted.advance(counted.make(big, "BlanesMoan6B"), 3)
    assert own >= 3 * 6
    with_big = [counted.make(a, "BlanesMoan6B"), counted.make(big, "BlanesMoan6B"), counted.make(c, "Ruth")]
    assert counted.advance_many(with_big, 3) == 1 + own and [counted.steps(h) for h in with_big] == [3] * 3
    # one plain and one <Double>: two groups of one, two launches of the single-system kernels
    assert counted.advance_many([counted.make(a, "Ruth"), counted.make(a, "Ruth", True)], 5) == 2
    # a symplectic pair beside a multistep pair: each kind its own launches (start-up gang, and the SRKN gang)
    beside = [counted.make(a, "QuinlanTremaine12"), counted.make(a, "Ruth"), counted.make(b, "QuinlanTremaine12"), counted.make(b, "Ruth")]
    assert counted.advance_many(beside, 12) == 2 and [counted.steps(h) for h in beside] == [12] * 4


@KINDS
def test_a_timed_member_that_is_not_the_lead(gpu, compensated):
    """kernel_time()[1] rises by one and the milliseconds stay: the lead alone times the shared launch"""
    m = gs.edge_member(17, 1)
    gang = [m.make(gpu.NBodyIntegration, ss.FSAL_TABLE, compensated=compensated) for _ in range(3)]
    lead, other = gs.LaunchProbe(gang[0]), gs.LaunchProbe(gang[2])
    gpu.advance_many(gang, 11)
    for g in gang:
        g.sync()
    ms, launches = lead.after_call()
    assert launches == 1 and ms > 0.0, (launches, ms)
    other.assert_ganged("three members, advance_many(11), member 2")
    with Order(gpu, gpu.pair_variant()):
        for j, g in enumerate(gang):
            assert_against_oracle(ss.record(g), gpu.pair_variant(), compensated, m, ss.FSAL_TABLE, 11, f"member {j}")


# ---- 3. per-member stops
@KINDS
@pytest.mark.parametrize("ordering", list(sg.STOP_ORDERS))
def test_every_member_stops_at_its_own_bound(gpu, ordering, compensated):
    """bounds that leave 0, 1, 3, exactly k and more than k steps, and a member whose t + h == t, in one call: the status is the
    first in member order; every member is where its own advance(k) leaves it; behind the lifted bounds the gang goes on"""
    with Order(gpu, 0):
        scene = [sg.stop_members()[j] for j in sg.STOP_ORDERS[ordering]]
        gang, alone = ([m.make(gpu.NBodyIntegration, compensated=compensated) for m in scene] for _ in range(2))
        oracles = [m.make(orc.NBody) for m in scene]
        probe = gs.LaunchProbe(gang[[m.name for m in scene].index("exactly")])
        assert [m.name for m in scene].index("exactly") != 0 and scene[0].steps > 0
        assert status_of(lambda: gpu.advance_many(gang, sg.STOP_K)) == sg.first_status(sg.stop_members(), sg.STOP_ORDERS[ordering])
        probe.assert_ganged(f"{ordering}: the member that takes exactly k steps")
        for call, k in enumerate((sg.STOP_K, sg.STOP_FOLLOW_UP)):
            if call:
                for h in gang + alone + oracles:
                    h.set_bound(INF)
                assert status_of(lambda: gpu.advance_many(gang, k)) == sg.STEP_SIZE_UNDERFLOW      # that member stays where it is
                probe.assert_ganged(f"{ordering}: behind the lifted bounds")
            for m, g, a, o in zip(scene, gang, alone, oracles):
                where = f"{ordering}, {'<Double>' if compensated else 'plain'}: {m.name}, call {call}"
                want = m.status if not call else sg.STEP_SIZE_UNDERFLOW if m.name == "underflow" else 0
                assert status_of(lambda: a.advance(k)) == want and o.advance(k) == want, where
                rec = ss.record(g)
                assert int(rec["steps"][0]) == (m.steps if not call else m.steps + k if m.name != "underflow" else 0), where
                assert_record(rec, ss.record(a), f"{where}: against the twin advanced alone")
                if not compensated:
                    assert_record(rec, ss.record(o), f"{where}: against orc.NBody")
                else:                                                    # the scalar bookkeeping is the plain oracle's too
                    assert_record(rec, ss.record(o), f"{where}: against orc.NBody", keys=("t", "steps", "evals"))


# ---- 4. more workgroups than CUs
@KINDS
def test_more_workgroups_than_compute_units(gpu, compensated):
    """(CU count + 8) members of 3 bodies, clones of four distinct entry states, k = 7: clones entered equal are equal, and the four
    are the oracle's"""
    hip, dev, count = gpu.hip_runtime(), C.c_int(-1), C.c_int(0)
    assert hip.hipGetDevice(C.byref(dev)) == 0 and hip.hipDeviceGetAttribute(C.byref(count), 63, dev) == 0   # multiprocessor count
    assert 64 <= count.value <= 512, count.value
    m = sg.clone_source()
    with Order(gpu, gpu.pair_variant()):
        sources = [m.make(gpu.NBodyIntegration, sg.CLONE_TABLE, compensated=compensated) for _ in sg.CLONE_ENTRIES]
        for g, entry in zip(sources, sg.CLONE_ENTRIES):
            if entry:
                g.advance(entry)
        gang = sources + [sources[j % 4].clone() for j in range(4, count.value + 8)]
        probe = gs.LaunchProbe(gang[-1])
        gpu.advance_many(gang, sg.CLONE_K)
        probe.assert_ganged(f"gang of {len(gang)}, the last member")
        want = [ss.record(g) for g in sources]
        for j, entry in enumerate(sg.CLONE_ENTRIES):
            assert_against_oracle(want[j], gpu.pair_variant(), compensated, m, sg.CLONE_TABLE, entry + sg.CLONE_K, f"source {j}")
        for j, g in enumerate(gang[4:], 4):
            assert_record(ss.record(g), want[j % 4], f"member {j} of {len(gang)} against its source")


# ---- 5. sampled
def _sampled_run(members, table, make, many):
    """gs.SAMPLED_CALLS on the propagators of `members`, through many(props, k) where given, else step_n(k) on each; a take after
    every call -> per member, the list of (what, arrays) that ss.compare_sampled takes"""
    props = [m.make(make, table) for m in members]
    out = [[] for _ in members]
    for k in gs.SAMPLED_CALLS:
        if many:
            many(props, k)
        else:
            for m, p in zip(members, props):
                assert p.step_n(k) in (None, 0), (m.name, k)
        for m, p, recs in zip(members, props, out):
            rec = ss._take(p, m.n)
            pos, vel, t, c = p.state()
            rec.update(pos=np.array(pos), vel=np.array(vel), steps=np.array([c], dtype=np.int64))
            recs.append((f"after step_n({k})", rec))
    return out


_sampled_oracle = {}


@pytest.mark.parametrize("table", ss.SAMPLED_TABLES)
def test_sampled_propagators_share_their_launches(gpu, table):
    """step_n_many on the sampled members (3 and 32 bodies forward, 17 backward): the kernel's countdown is each member's own"""
    members = ss.sampled_members()
    with Order(gpu, 0):
        if table not in _sampled_oracle:
            _sampled_oracle[table] = _sampled_run(members, table, orc.Propagator, None)
        make = lambda *a: gpu.NBodyPropagator(*a[:8], method=a[8])
        probes = {}

        def many(props, k):
            if not probes:
                probes[1] = gs.LaunchProbe(props[1].integration())
            gpu.step_n_many(props, k)
            probes[1].assert_ganged(f"{table}: step_n_many({k}), the 17-body member")        # every call here is one chunk: one launch
        got = _sampled_run(members, table, make, many)
        alone = _sampled_run(members, table, make, None)
        for m, g, a, w in zip(members, got, alone, _sampled_oracle[table]):
            ss.compare_sampled(g, w, f"{table}, {m.name}: step_n_many against orc.Propagator")
            ss.compare_sampled(g, a, f"{table}, {m.name}: step_n_many against step_n")
            assert (g[-1][1]["npoly"] > 0).all(), (table, m.name)


# ---- 6. allocation failure
@KINDS
def test_the_first_gang_under_a_failing_allocation(gpu, hooks, counted, compensated):
    """the lead's argument array is the call's one allocation: with it failing the call returns out-of-memory and nobody has moved;
    the same call then succeeds, and the members are where twins are that never saw a failure"""
    scene = [(gs.edge_member(17, 1), "BlanesMoan6B", 0), (gs.edge_member(32, -1), "McLachlanO4", 2), (gs.edge_member(3, 1), "BlanesMoan14A", 1)]
    gang, twins = ([counted.make(m, table, compensated) for m, table, _ in scene] for _ in range(2))
    for hs in (gang, twins):
        for h, (_, _, entry) in zip(hs, scene):
            if entry:
                counted.advance(h, entry)
    arr = (C.c_void_p * len(gang))(*[h.value for h in gang])

    def call():
        return counted.L.eph_nbody_advance_many(arr, len(gang), 9), None, counted.L.eph_last_error().decode()

    def failed(k, out):
        for h, t, (m, table, _) in zip(gang, twins, scene):
            assert_record(counted.record(h, m.n), counted.record(t, m.n), f"allocation {k} failing: {m.name} has not moved")
    failures, _ = failing_allocations(gpu, hooks, call, failed)
    assert failures == 1
    for t in twins:
        counted.advance(t, 9)
    for h, t, (m, table, entry) in zip(gang, twins, scene):
        rec = counted.record(h, m.n)
        assert int(rec["steps"][0]) == entry + 9
        assert_record(rec, counted.record(t, m.n), f"the retried call: {m.name}")
    assert counted.advance_many(gang, 4) == 1                                # (the array is there now: no allocation, one launch)


def test_a_failing_allocation_in_the_second_launch_of_a_call(gpu, hooks, counted):
    """two plain and two <Double> members are two launches, each with its lead's array. With the SECOND allocation failing the call
    returns out-of-memory behind the plain launch: the plain members have advanced, the <Double> ones have not moved, nobody is
    failed for good (include/ephemeris_amd.h says so of eph_nbody_advance_many)"""
    m, table = gs.edge_member(17, 1), "BlanesMoan6B"
    kinds = (False, False, True, True)
    gang, twins = ([counted.make(m, table, c) for c in kinds] for _ in range(2))
    arr = (C.c_void_p * len(gang))(*[h.value for h in gang])
    assert hooks.fail_alloc(2) == 0
    st, text = counted.L.eph_nbody_advance_many(arr, len(gang), 5), counted.L.eph_last_error().decode()
    assert hooks.fail_alloc(0) == 0 and st == gpu.ERR_OUT_OF_MEMORY and "injected allocation failure" in text, (st, text)
    for t in twins[:2]:
        counted.advance(t, 5)
    for j, (h, t) in enumerate(zip(gang, twins)):
        rec = counted.record(h, m.n)
        assert int(rec["steps"][0]) == (0 if kinds[j] else 5), j
        assert_record(rec, counted.record(t, m.n), f"behind the failure: member {j}")
    assert counted.advance_many(gang, 3) == 2
    for t in twins:
        counted.advance(t, 3)
    for j, (h, t) in enumerate(zip(gang, twins)):
        assert_record(counted.record(h, m.n), counted.record(t, m.n), f"the call behind the failure: member {j}")


# ---- 7. the convergence sweep, side by side
class SweepLaunches:
    """The steady-state launches that the runs of a sweep queue, counted from inside convergence() / convergence_gang() themselves:
    the package's advance_many and NBodyIntegration.advance are wrapped while the block runs. Every run is timed, so that
    eph_nbody_kernel_time counts its launches; in a shared launch the lead counts it with milliseconds of its own, every other
    member counts it with none (gs.LaunchProbe)."""

    def __init__(self, gpu, monkeypatch):
        self.launches, self.gangs = 0, []
        real_advance, real_many = gpu.NBodyIntegration.advance, gpu.advance_many

        def advance(g, n_steps=1):
            g.enable_timing()
            before = g.kernel_time()[1]
            try:
                real_advance(g, n_steps)
            finally:
                self.launches += g.kernel_time()[1] - before

        def advance_many(runs, n_steps):
            probes = [gs.LaunchProbe(g) for g in runs]
            try:
                real_many(runs, n_steps)
            finally:
                ms, launches = probes[0].after_call()
                assert launches == 1 and ms > 0.0, f"the lead of {len(runs)} runs: {launches} launches, {ms} ms"
                for j, p in enumerate(probes[1:], 1):
                    p.assert_ganged(f"run {j} of {len(runs)} side by side")
                self.launches += 1
                self.gangs.append(len(runs))
        monkeypatch.setattr(gpu.NBodyIntegration, "advance", advance)
        monkeypatch.setattr(gpu, "advance_many", advance_many)


def test_convergence_gang_equals_convergence(gpu, monkeypatch):
    """the shipped 10-body system, McLachlanO4, ten days from h0 = 300 s: answer and rows of convergence_gang() are those of
    convergence() bit for bit (and the oracle's), and it queues fewer launches: one per batch of runs against one per run"""
    from ephemeris_explorer_amd.convergence import GANG_CANDIDATES                    # (the package's `convergence` is the function)
    s = load_system(sg.SWEEP["system"])
    bound = s.epoch + sg.SWEEP["days"] * 86400.0
    args = (s.pos, s.vel, s.mu, s.epoch, bound, sg.SWEEP["method"], sg.SWEEP["h0"])
    with monkeypatch.context() as m:
        seq = SweepLaunches(gpu, m)
        h_seq, rows_seq = gpu.convergence(*args)
    with monkeypatch.context() as m:
        gang = SweepLaunches(gpu, m)
        h_gang, rows_gang = gpu.convergence_gang(*args)
    assert h_gang == h_seq and rows_gang.shape == rows_seq.shape and np.array_equal(bits(rows_gang), bits(rows_seq)), (rows_gang, rows_seq)
    assert len(rows_seq) >= 3 and sg.sweep_steps(rows_seq, bound - s.epoch, sg.SWEEP["h0"]) < sg.SWEEP_STEP_LIMIT
    orc.set_pair_variant(gpu.pair_variant())
    try:
        h_orc, rows_orc = orc.convergence(*args)
    finally:
        orc.set_pair_variant(0)
    assert h_orc == h_seq and np.array_equal(bits(rows_orc), bits(rows_seq))
    runs = 1 + len(rows_seq)
    assert seq.gangs == [] and seq.launches == runs                                   # one launch per run, the truth run's among them
    # the truth run with the first candidates, then the next candidates; a member's own advance(1) afterwards queued nothing
    assert gang.gangs == [1 + GANG_CANDIDATES] + [GANG_CANDIDATES] * (len(gang.gangs) - 1) and sum(gang.gangs) >= runs
    assert gang.launches == len(gang.gangs) < seq.launches, (gang.launches, gang.gangs, seq.launches)
