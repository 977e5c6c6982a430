"""-m gpu: the multistep start-up of at most 32 bodies in one launch (k_lm_startup_small, csrc/step_srkn_small.hip), alone and as a
gang of eph_nbody_advance_many / eph_prop_step_n_many, on the scenes of tests/startup_scenes.py.

Every comparison is on bit patterns through the C ABI: against orc.NBody / orc.Propagator / the oracle's Double solver, and against a
second device handle on set_path(1), whose start-up is the per-launch one. No tolerance appears anywhere.

Which route ran cannot be told from bits -- the routes are built to agree -- and the boundary has no call for it (its function list
is pinned by the ABI tests). The launch-count tests at the end therefore drive the test-hooks library (tests/hooks.py: the product's
objects and the eph_debug_* hooks), whose eph_debug_wg_cycles reports in a product build the kernel launches that advance /
advance_many have queued on this thread (csrc/eph_debug.h): a shared launch of a gang counts once there. The bound and underflow
scenes run through the fallback and assert bits only."""
import numpy as np
import pytest

import gang_scenes as gs
import startup_scenes as ss
from oracle import orc

pytestmark = pytest.mark.gpu

INF = float("inf")
SCENES = {s.name: s for s in ss.scenes()}
BOUNDS = {s.name: s for s, _ in ss.bound_scenes()}


@pytest.fixture(scope="module", autouse=True)
def oracle_order(gpu):
    """the oracle evaluates the point-mass term in the order the device's handles take"""
    orc.set_pair_variant(gpu.pair_variant())
    yield
    orc.set_pair_variant(0)


_trails = {}


def oracle_play(scene, method, calls):
    """orc.NBody's (status, record) after every call, computed once per (scene, method, calls) and left unchanged"""
    key = (scene.name, method, tuple(calls))
    if key not in _trails:
        _trails[key] = ss.play(scene.make(orc.NBody, method), calls)
    return _trails[key]


def double_play(scene, method, calls):
    """the same from the oracle's Double solver: value parts, time and step count after every call"""
    out, done = [], 0
    for k in calls:
        done += k
        st, y, dy, end = orc.double_solve(scene.pos, scene.vel, scene.mu, scene.t0, INF, scene.h, method, max_steps=done)
        assert st == 0
        out.append((0, dict(pos=y[..., 0].copy(), vel=dy[..., 0].copy(), t=np.array([end]), steps=np.array([done], dtype=np.int64))))
    return out


@pytest.mark.parametrize("compensated", [False, True], ids=["plain", "double"])
@pytest.mark.parametrize("method", list(ss.METHODS))
@pytest.mark.parametrize("name", list(SCENES))
def test_the_plan_on_every_scene(gpu, name, method, compensated):
    """advance(1), advance(4), advance(L), advance(2 L + 5): state, acc(), time, step count and eval_count() after every call"""
    scene, calls = SCENES[name], ss.plan(ss.METHODS[method])
    got = ss.play(scene.make(gpu.NBodyIntegration, method, compensated=compensated), calls)
    per_launch = scene.make(gpu.NBodyIntegration, method, compensated=compensated)
    per_launch.set_path(1)
    ss.assert_plays(got, ss.play(per_launch, calls), f"{name}, {method}: against path 1")
    want = double_play(scene, method, calls) if compensated else oracle_play(scene, method, calls)
    ss.assert_plays(got, want, f"{name}, {method}: against the oracle")
    assert got[1][1]["evals"][0] < ss.startup_evals(ss.METHODS[method]) == got[2][1]["evals"][0] - 5


@pytest.mark.parametrize("method", list(ss.METHODS))
@pytest.mark.parametrize("name", list(BOUNDS))
def test_route_changing_scenes(gpu, name, method):
    """a bound that fires on a substep of macro step 5, one exactly on a macro boundary, a step that underflows at once: status,
    state, acc(), time and counters are the oracle's after every call of the plan"""
    scene, calls = BOUNDS[name], ss.plan(ss.METHODS[method])
    want = oracle_play(scene, method, calls)
    assert {st for st, _ in want} - {0} == {dict((s.name, w) for s, w in ss.bound_scenes())[name]}
    for compensated in (False, True):
        got = ss.play(scene.make(gpu.NBodyIntegration, method, compensated=compensated), calls)
        if not compensated:
            ss.assert_plays(got, want, f"{name}, {method}: against the oracle")
        per_launch = scene.make(gpu.NBodyIntegration, method, compensated=compensated)
        per_launch.set_path(1)
        ss.assert_plays(got, ss.play(per_launch, calls), f"{name}, {method}, compensated={compensated}: against path 1")
        assert [st for st, _ in got] == [st for st, _ in want]
        for (_, g), (_, w) in zip(got, want):
            assert g["t"][0] == w["t"][0] and g["steps"][0] == w["steps"][0] and g["evals"][0] == w["evals"][0]


@pytest.mark.parametrize("compensated", [False, True], ids=["plain", "double"])
@pytest.mark.parametrize("method", list(ss.METHODS))
def test_a_clone_taken_in_mid_start_up_continues(gpu, method, compensated):
    L, scene = ss.METHODS[method], SCENES["plummer17+"]
    g = scene.make(gpu.NBodyIntegration, method, compensated=compensated)
    g.advance(5)
    c = g.clone()
    calls = (3, L, 7)
    got, twin = ss.play(c, calls), ss.play(g, calls)
    ss.assert_plays(got, twin, f"{method}: the clone against its source")
    whole = (5,) + calls
    want = double_play(scene, method, whole)[1:] if compensated else oracle_play(scene, method, whole)[1:]
    ss.assert_plays(got, want, f"{method}: the clone against the oracle")


# ---- sampled
def sampled_members():
    return [gs.SampledMember(n, d) for n in (3, 17, 32) for d in (gs.FORWARD, gs.BACKWARD)]


def sampled_record(p, n):
    rec = gs.sampled_record(p, n)
    rec["t"] = np.array([rec["t"][0], rec["t"][1], p.integrator_time()])
    return rec


_sampled = {}


def oracle_sampled(method):
    """orc.Propagator's records after every call of the plan, per member; computed once"""
    if method not in _sampled:
        out = []
        for m in sampled_members():
            o, recs = m.make(orc.Propagator, method), []
            for k in ss.plan(ss.METHODS[method]):
                assert o.step_n(k) == 0
                recs.append(sampled_record(o, m.n))
            out.append(recs)
        _sampled[method] = out
    return _sampled[method]


@pytest.mark.parametrize("ganged", [False, True], ids=["step_n", "step_n_many"])
@pytest.mark.parametrize("method", list(ss.METHODS))
def test_sampled_propagators_across_the_start_up(gpu, method, ganged):
    """step_n in the pieces of the plan, take_solution after each: polynomials, spline bounds, time() and integrator_time()"""
    members = sampled_members()
    props = [m.make(gpu.NBodyPropagator, method) for m in members]
    want = oracle_sampled(method)
    for c, k in enumerate(ss.plan(ss.METHODS[method])):
        if ganged:
            gpu.step_n_many(props, k)
        else:
            for p in props:
                p.step_n(k)
        gs.compare_sampled(members, [sampled_record(p, m.n) for m, p in zip(members, props)], [w[c] for w in want],
                           f"{method}, {'ganged' if ganged else 'alone'}, after call {c}")


# ---- ganged
def gang_scenes():
    """nine members: every size, a backward and a massless one among them"""
    return [SCENES[f"plummer{n}+"] for n in ss.SIZES] + [SCENES["plummer32-"], SCENES["plummer17--massless"]]


@pytest.mark.parametrize("method", list(ss.METHODS))
def test_a_fresh_gang_of_every_size(gpu, method):
    scenes, calls = gang_scenes(), ss.plan(ss.METHODS[method])
    assert len(scenes) == 9
    gang = [s.make(gpu.NBodyIntegration, method) for s in scenes]
    alone = [s.make(gpu.NBodyIntegration, method) for s in scenes]
    for c, k in enumerate(calls):
        gpu.advance_many(gang, k)
        for s, g, a in zip(scenes, gang, alone):
            rec = ss.record(g)
            assert ss.status_of(a, k) == 0
            ss.assert_same(rec, ss.record(a), f"{method}: ganged call {c}, {s.name}: against the member alone")
            ss.assert_same(rec, oracle_play(s, method, calls)[c][1], f"{method}: ganged call {c}, {s.name}: against the oracle")


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "with-33-bodies-and-a-double"])
@pytest.mark.parametrize("method", list(ss.METHODS))
def test_a_gang_whose_members_are_at_different_points_of_their_start_up(gpu, method, mixed):
    """members that have taken 0, 1, 5 and L - 1 macro steps alone: m_i = L, L - 1, L - 5 and 1 of k = L + 5, unequal remainders;
    then a second call, all steady. Mixed: a 33-body member and a <Double> member go the separate way inside the same call"""
    L = ss.METHODS[method]
    taken = (0, 1, 5, L - 1)
    scenes = [SCENES["plummer32+"], SCENES["plummer17+"], SCENES["plummer31+"], SCENES["plummer3+"]]
    gang = [s.make(gpu.NBodyIntegration, method) for s in scenes]
    for g, t in zip(gang, taken):
        if t:
            g.advance(t)
    extra = []
    if mixed:
        big = ss.sphere(ss.FIRST_PER_LAUNCH_SIZE)
        extra = [(big, big.make(gpu.NBodyIntegration, method), False),
                 (SCENES["plummer16+"], SCENES["plummer16+"].make(gpu.NBodyIntegration, method, compensated=True), True)]
    handles = gang[:2] + [h for _, h, _ in extra] + gang[2:]
    for c, k in enumerate((L + 5, 7)):
        gpu.advance_many(handles, k)
        for s, g, t in zip(scenes, gang, taken):
            calls = ((t,) if t else ()) + (L + 5, 7)
            want = oracle_play(s, method, calls)[c + (1 if t else 0)][1]
            ss.assert_same(ss.record(g), want, f"{method}: call {c}, {s.name} entered after {t} steps")
        for s, h, compensated in extra:
            if compensated:
                want = double_play(s, method, (L + 5, 7))[c][1]
            else:
                want = oracle_play(s, method, (L + 5, 7))[c][1]
            ss.assert_same(ss.record(h), want, f"{method}: call {c}, {s.name} (compensated={compensated})")


def test_more_workgroups_than_can_be_resident(gpu):
    """(CU count + 8) clones of a fresh 3-body handle, k = L + 5: every member equals the first, and the first the oracle"""
    import ctypes as C
    hip, dev, count = gpu.hip_runtime(), C.c_int(-1), C.c_int(0)
    assert hip.hipGetDevice(C.byref(dev)) == 0 and hip.hipDeviceGetAttribute(C.byref(count), 63, dev) == 0   # multiprocessor count
    assert 64 <= count.value <= 512, count.value
    method, L, scene = "QuinlanTremaine12", 12, SCENES["sun_earth_moon"]
    first = scene.make(gpu.NBodyIntegration, method)
    gang = [first] + [first.clone() for _ in range(count.value + 7)]
    gpu.advance_many(gang, L + 5)
    want = ss.record(first)
    ss.assert_same(want, oracle_play(scene, method, (L + 5,))[0][1], "the first member against the oracle")
    for j, g in enumerate(gang[1:], 1):
        ss.assert_same(ss.record(g), want, f"member {j} of {len(gang)}")


def test_33_bodies_and_the_timed_handle(gpu):
    """33 bodies keep the per-launch start-up, plain and <Double>, with the oracle's bits; eph_nbody_kernel_time keeps counting the
    steady-state kernels only: one after a timed fresh advance(L + 5)"""
    big = ss.sphere(ss.FIRST_PER_LAUNCH_SIZE)
    for compensated in (False, True):
        got = ss.play(big.make(gpu.NBodyIntegration, "QuinlanTremaine12", compensated=compensated), (12, 5))
        want = double_play(big, "QuinlanTremaine12", (12, 5)) if compensated else oracle_play(big, "QuinlanTremaine12", (12, 5))
        ss.assert_plays(got, want, f"33 bodies, compensated={compensated}")
        g = SCENES["full_solar_system"].make(gpu.NBodyIntegration, "QuinlanTremaine12", compensated=compensated)
        g.enable_timing()
        g.advance(12 + 5)
        g.sync()
        assert g.kernel_time()[1] == 1 and g.eval_count() == ss.startup_evals(12) + 5


@pytest.mark.parametrize("method", list(ss.METHODS))
def test_a_timed_gang_across_the_start_up(gpu, method):
    """three fresh plain members, timing on the lead and on one other, advance_many(L + 5): eph_nbody_kernel_time keeps counting the
    steady-state kernels only in a gang too. Both gain ONE launch, the steady one; the lead times it, the other member gains no
    milliseconds of its own (gs.LaunchProbe); every member has the oracle's bits"""
    L, scene = ss.METHODS[method], SCENES["sun_earth_moon"]
    gang = [scene.make(gpu.NBodyIntegration, method) for _ in range(3)]
    lead, other = gs.LaunchProbe(gang[0]), gs.LaunchProbe(gang[2])
    gpu.advance_many(gang, L + 5)
    for g in gang:
        g.sync()
    ms, launches = lead.after_call()
    assert launches == 1 and ms > 0.0, f"{method}: the lead: {launches} launches, {ms} ms"
    other.assert_ganged(f"{method}: fresh gang of 3, advance_many(L + 5), member 2")
    want = oracle_play(scene, method, (L + 5,))[0][1]
    for j, g in enumerate(gang):
        ss.assert_same(ss.record(g), want, f"{method}: member {j} against the oracle")


# ---- launch counts: what fails without the one-launch start-up
class Counted:
    """the handles of the launch-count tests, made in the test-hooks library (the count is that library's own), and its count"""

    def __init__(self, hooks):
        import ctypes as C
        self.C, self.H, L = C, hooks, hooks.L
        dp, vp = C.POINTER(C.c_double), C.c_void_p
        L.eph_nbody_create.argtypes = [C.c_int32, dp, dp, dp, C.c_double, C.c_double, C.c_char_p, C.POINTER(vp)]
        L.eph_nbody_advance.argtypes = [vp, C.c_int64]
        L.eph_nbody_advance_many.argtypes = [C.POINTER(vp), C.c_int32, C.c_int64]
        L.eph_nbody_set_path.argtypes = [vp, C.c_int32]
        L.eph_nbody_sync.argtypes = [vp]
        L.eph_nbody_get_state.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_uint32)]
        L.eph_nbody_destroy.argtypes = [vp]
        L.eph_nbody_destroy.restype = None
        self.L, self.made = L, []

    def count(self):
        return self.H.debug_wg_cycles()[0]

    def fresh(self, scene, method, compensated=False, path=0):
        C, h = self.C, self.C.c_void_p()
        as_dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
        name = (method + ("<Double>" if compensated else "")).encode()
        assert self.L.eph_nbody_create(scene.n, as_dp(scene.pos), as_dp(scene.vel), as_dp(scene.mu), scene.t0, scene.h, name, C.byref(h)) == 0
        assert self.L.eph_nbody_set_path(h, path) == 0
        self.made.append(h)
        return h

    def advance(self, h, k):
        """launches queued by advance(k)"""
        before = self.count()
        assert self.L.eph_nbody_advance(h, k) == 0 and self.L.eph_nbody_sync(h) == 0
        return self.count() - before

    def advance_many(self, hs, k):
        before = self.count()
        arr = (self.C.c_void_p * len(hs))(*[h.value for h in hs])
        assert self.L.eph_nbody_advance_many(arr, len(hs), k) == 0
        for h in hs:
            assert self.L.eph_nbody_sync(h) == 0
        return self.count() - before

    def steps(self, h):
        c = self.C.c_uint32()
        assert self.L.eph_nbody_get_state(h, None, None, None, self.C.byref(c)) == 0
        return c.value

    def close(self):
        for h in self.made:
            self.L.eph_nbody_destroy(h)
        self.made = []


@pytest.fixture
def counted(hooks):
    c = Counted(hooks)
    yield c
    c.close()


@pytest.mark.parametrize("method", list(ss.METHODS))
@pytest.mark.parametrize("compensated", [False, True], ids=["plain", "double"])
def test_launch_counts_of_a_fresh_32_body_handle(counted, method, compensated):
    """path 0: advance(L) is ONE launch, a fresh advance(L + 5) two; path 1: every force evaluation is a launch"""
    L, scene = ss.METHODS[method], SCENES["full_solar_system"]
    assert counted.advance(counted.fresh(scene, method, compensated), L) == 1
    assert counted.advance(counted.fresh(scene, method, compensated), L + 5) == 2
    cut = counted.fresh(scene, method, compensated)        # the plan: start-up launches of m = 1, 4 and L - 5, then steady ones
    assert [counted.advance(cut, k) for k in ss.plan(L)] == [1, 1, 2, 1]
    assert counted.advance(counted.fresh(scene, method, compensated, path=1), L) >= ss.startup_evals(L)


@pytest.mark.parametrize("method", list(ss.METHODS))
def test_launch_counts_of_a_fresh_gang(counted, method):
    """three fresh plain members: advance_many(L) is ONE launch for all of them, a fresh advance_many(L + 5) two; members at
    different points of their start-up share the start-up launch and finish their unequal remainders alone"""
    L, scene = ss.METHODS[method], SCENES["full_solar_system"]
    gang = [counted.fresh(scene, method) for _ in range(3)]
    assert counted.advance_many(gang, L) == 1 and [counted.steps(h) for h in gang] == [L] * 3
    gang = [counted.fresh(scene, method) for _ in range(3)]
    assert counted.advance_many(gang, L + 5) == 2 and [counted.steps(h) for h in gang] == [L + 5] * 3
    gang = [counted.fresh(scene, method) for _ in range(4)]
    for h, t in zip(gang, (0, 1, 5, L - 1)):
        if t:
            assert counted.advance(h, t) == 1
    assert counted.advance_many(gang, L + 5) == 1 + 4
    assert counted.advance_many(gang, 7) == 1
    # a <Double> member takes its own one-launch start-up beside the gang's
    gang = [counted.fresh(scene, method), counted.fresh(scene, method, compensated=True), counted.fresh(scene, method)]
    assert counted.advance_many(gang, L) == 2


def test_launch_counts_where_the_per_launch_route_stays(counted):
    """33 bodies: in the hundreds, plain and <Double>; a bound inside the start-up: the whole call goes per launch"""
    big = ss.sphere(ss.FIRST_PER_LAUNCH_SIZE)
    for compensated in (False, True):
        assert 302 <= counted.advance(counted.fresh(big, "QuinlanTremaine12", compensated), 12) < 1000
    scene = BOUNDS["bound-on-boundary"]
    h = counted.fresh(scene, "QuinlanTremaine12")
    assert counted.L.eph_nbody_set_bound(h, counted.C.c_double(scene.bound)) == 0
    assert counted.advance(h, 4) == 1                      # four macro steps in front of the bound: one launch
    before = counted.count()
    assert counted.L.eph_nbody_advance(h, 4) == ss.BOUND_REACHED and counted.steps(h) == 5
    assert counted.count() - before == 30                  # one macro step on the per-launch route, then the bound's test
