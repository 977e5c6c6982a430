"""-m gpu: the lifecycle calls of the N-body host side (csrc/nbody.cpp, csrc/propagator.cpp) under a failing allocation, and the
read-back through its NULL arguments. eph_nbody_create, eph_nbody_clone, the first steady batch of the fast paths, eph_prop_clone,
eph_prop_step_n and the first eph_nbody_advance_many of a steady and of a fresh gang are walked with the k-th device allocation failing for k = 1, 2, ... (eph_debug_fail_alloc: a host function returns
EPH_ERR_OUT_OF_MEMORY before any HIP call; nothing is provoked on the device). After every failure the objects involved go on bit for
bit like twins that never saw one. No tolerance anywhere.

Each case is one child process (this file run as a script) on the test-hooks library, under its own timeout; after a child that died
of a signal or ran into its timeout no further child is started. Every case asserts how many device allocations its call makes
(ALLOCATIONS, measured on the commit before the handle's buffers were stated once: profiles/nbody_host_frame.md; the two gang cases
on the commit before the gangs shared one launch frame: profiles/gang_frame.md): a buffer dropped from, or added to, a walk over the
statement of NBodyIntegration's buffers moves a count.

The sharded read-back is tests/test_gpu_shard.py's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gang_scenes import H, random_system
from hooks import failing_allocations

pytestmark = pytest.mark.gpu

HOOKS_LIB = ROOT / "ephemeris_explorer_amd" / "libephemeris_amd_testhooks.so"
METHOD, STARTUP = "QuinlanTremaine12", 12
SRKN = "BlanesMoan6B"
DOUBLE = "<Double>"
UNTOUCHED = 0x5A5A5A5A
_dead_children = []

# Device allocations of each call: the number of k at which it fails before it first succeeds.
ALLOCATIONS = {"create": 8,            # P_[0], P_[1], Y_, A_, V_, ASR_, mu_, stage_
               "create-double": 10,    # and YE_, VE_
               "clone": 8, "clone-double": 10,
               "first-batch-fast": 1,  # fast_partial_
               "first-batch-f32": 2,   # fast_partial_, posf_
               "prop-clone": 14,       # the integration's 8, log_, d_period_, d_phase_, d_offset_, pend_co_, pend_nc_
               "prop-step-fit": 5,     # d_first_, d_deg_, d_src_, d_cnt_, d_region_ (a failed pending list spills and retries: no failure)
               "prop-step-advance": 1, # fast_partial_ (the steady batch's fit reuses the start-up's scratch)
               "gang-steady": 1,       # the lead's LmArgs array
               "gang-startup": 1,      # the lead's LmStartupArgs array
               "read-back": 0}
counted = {}


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def last_error(ea):
    return ea._lib().eph_last_error().decode()


def same_state(a, b, what):
    (pa, va, ta, ca), (pb, vb, tb, cb) = a.state(), b.state()
    assert ta == tb and ca == cb, (what, ta, tb, ca, cb)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb), what
    assert np.array_equal(a.acc(), b.acc()), what
    return ca


def same_solution(sa, sb, n, what):
    for b in range(n):
        assert sa.info(b) == sb.info(b), (what, b, sa.info(b), sb.info(b))
        (ca, na), (cb, nb) = sa.coeffs(b), sb.coeffs(b)
        assert np.array_equal(na, nb) and np.array_equal(ca, cb), (what, b)
    return sum(sa.info(b)[2] for b in range(n))


def integration(ea, n, method=METHOD, steps=0, path=0):
    g = ea.NBodyIntegration(*random_system(n), 0.0, H, method)
    if path:
        g.set_path(path)
    g.advance(steps)
    return g


def propagator(ea, n, steps, path=0):
    count, degree = np.ones(n, np.uint32), (3 + np.arange(n) % 5).astype(np.uint32)      # a sample every step: a window every 8
    p = ea.NBodyPropagator(*random_system(n), 0.0, H, ea.FORWARD, count, degree)
    p.step_n(steps)
    if path:
        p.integration().set_path(path)
    return p


def raw_new(ea, name, *args):
    """eph_*(*args, &out) -> (status, out or None, the error text)"""
    out = C.c_void_p(UNTOUCHED)
    st = getattr(ea._lib(), name)(*args, C.byref(out))
    return st, out.value, last_error(ea)


# ---- 1. eph_nbody_create ------------------------------------------------------------------------------------------------------------
def create_case(ea, H_, tag):
    pos, vel, mu = (ea._f64(a) for a in random_system(3))
    method = (METHOD + tag).encode()

    def failed(k, out):
        assert out is None, (k, out)                                      # eph_nbody_create clears *out before anything can fail
    failures, out = failing_allocations(ea, H_, lambda: raw_new(ea, "eph_nbody_create", 3, ea._p(pos), ea._p(vel), ea._p(mu), 0.0, H, method), failed)
    good = ea.NBodyIntegration._adopt(C.c_void_p(out), n=3, compensated=bool(tag))
    plain = ea.NBodyIntegration(pos, vel, mu, 0.0, H, METHOD + tag)
    for g in (good, plain):
        g.advance(20)
    assert same_state(good, plain, "created after the failures against a plain creation") == 20
    counted["create-double" if tag else "create"] = failures


# ---- 2. eph_nbody_clone -------------------------------------------------------------------------------------------------------------
def clone_case(ea, H_, tag):
    src, twin = (integration(ea, 3, METHOD + tag, STARTUP + 2) for _ in range(2))

    def failed(k, out):
        assert out is None, (k, out)
        for g in (src, twin):
            g.advance(1)
        same_state(src, twin, f"k = {k}: the source against its twin")
    failures, out = failing_allocations(ea, H_, lambda: raw_new(ea, "eph_nbody_clone", src._h), failed)
    good = ea.NBodyIntegration._adopt(C.c_void_p(out), n=3, compensated=bool(tag))
    same_state(good, src, "the clone at the clone")
    for g in (good, src, twin):
        g.advance(20)
    assert same_state(good, src, "the clone, 20 steps on") == STARTUP + 2 + failures + 20
    same_state(src, twin, "the source, 20 steps on")
    counted["clone-double" if tag else "clone"] = failures


# ---- 3. the first steady batch of a fast path: the lazy scratch ---------------------------------------------------------------------------
def first_batch_case(ea, H_, path, name):
    g, never = (integration(ea, 65, steps=STARTUP, path=path) for _ in range(2))          # 65: the smallest size above one workgroup's

    def failed(k, out):
        assert same_state(g, never, f"k = {k}: no step taken") == STARTUP
    failures, _ = failing_allocations(ea, H_, lambda: (ea._lib().eph_nbody_advance(g._h, 5), None, last_error(ea)), failed)
    never.advance(5)
    assert same_state(g, never, "the retried batch") == STARTUP + 5
    for x in (g, never):
        x.advance(3)
    same_state(g, never, "the batch after it")
    counted[name] = failures


# ---- 4. eph_prop_clone with pending device-resident windows --------------------------------------------------------------------------
def prop_clone_case(ea, H_):
    src, twin = (propagator(ea, 3, 20) for _ in range(2))                               # 2 windows per body wait on the device

    def failed(k, out):
        assert out is None, (k, out)
        for p in (src, twin):
            p.step_n(1)
        assert src.time() == twin.time()
    failures, out = failing_allocations(ea, H_, lambda: raw_new(ea, "eph_prop_clone", src._h), failed)
    good = ea.NBodyPropagator._adopt(C.c_void_p(out), n=3)
    same_state(good.integration(), src.integration(), "the clone at the clone")
    sg, ss, st = good.take_solution(), src.take_solution(), twin.take_solution()
    assert same_solution(ss, st, 3, "the source after the failures against its twin") >= 6
    same_solution(sg, ss, 3, "the clone against the source")
    for p in (good, src, twin):
        p.step_n(20)
    same_solution(good.take_solution(), src.take_solution(), 3, "the clone, 20 steps on")
    same_state(src.integration(), twin.integration(), "the source, 20 steps on")
    counted["prop-clone"] = failures


# ---- 5. eph_prop_step_n: sticky inside fit_and_push, returned inside the integrator's advance -------------------------------------------
def prop_step_fit_case(ea, H_):
    """the first batch that fits a window (step 8 of a sample per step). A failure there leaves the integrator one step ahead of the
    solout's bookkeeping: the propagator is failed for good, every later call returns the same status"""
    L = ea._lib()
    twin = propagator(ea, 3, 20)
    want = twin.take_solution()
    for k in range(1, 200):
        p = propagator(ea, 3, 7)
        assert H_.fail_alloc(k) == 0
        st = L.eph_prop_step_n(p._h, 1)
        text, left = last_error(ea), H_.fail_alloc(0)
        if st == ea.OK:
            # the pending list's two arrays come last. A refused one is no failure: the list spills to the host and is retried
            assert left == 0, f"k = {k}: allocation {k} was never reached"
            p.step_n(12)
            same_state(p.integration(), twin.integration(), f"k = {k}")
            assert same_solution(p.take_solution(), want, 3, f"k = {k}") == 6
            if counted.setdefault("prop-step-fit", k - 1) == k - 2:
                return
            continue
        assert "prop-step-fit" not in counted, f"k = {k} fails after k = {k - 1} succeeded"
        assert st == ea.ERR_OUT_OF_MEMORY and "injected allocation failure" in text and left == 0, (k, st, text, left)
        out = C.c_void_p(UNTOUCHED)
        assert L.eph_prop_step_n(p._h, 1) == st and L.eph_prop_step(p._h) == st and L.eph_prop_step_to(p._h, 1e9) == st, k
        assert L.eph_prop_take_solution(p._h, C.byref(out)) == st and out.value == UNTOUCHED, k
        assert raw_new(ea, "eph_prop_clone", p._h)[:2] == (st, None), k
    raise AssertionError("no success by k = 199")


def prop_step_advance_case(ea, H_):
    """the first steady batch on PATH_FAST: the failure is the integrator's, before fit_and_push has anything to do. It is returned and the
    propagator goes on"""
    p, twin = (propagator(ea, 65, STARTUP, path=ea.PATH_FAST) for _ in range(2))

    def failed(k, out):
        assert p.integration().state()[3] == STARTUP
    failures, _ = failing_allocations(ea, H_, lambda: (ea._lib().eph_prop_step_n(p._h, 8), None, last_error(ea)), failed)
    twin.step_n(8)
    assert same_state(p.integration(), twin.integration(), "the retried batch") == STARTUP + 8
    assert same_solution(p.take_solution(), twin.take_solution(), 65, "the retried batch") == 2 * 65
    counted["prop-step-advance"] = failures


# ---- 6. eph_nbody_advance_many: the argument array of the gang's lead ---------------------------------------------------------------------
def gang_case(ea, H_, name, entered, k):
    """three 3-body handles, member i entered after entered[i] steps alone; their first advance_many(k). A failure leaves every member
    where it was and none failed for good: the retry succeeds, and the members go on like twins that never saw a failure"""
    gang, twins = ([integration(ea, 3, steps=s) for s in entered] for _ in range(2))
    arr = (C.c_void_p * len(gang))(*[g._h for g in gang])

    def failed(f, out):
        for i, (g, t) in enumerate(zip(gang, twins)):
            assert same_state(g, t, f"k = {f}: member {i} has not moved") == entered[i]
    failures, _ = failing_allocations(ea, H_, lambda: (ea._lib().eph_nbody_advance_many(arr, len(gang), k), None, last_error(ea)), failed)
    ea.advance_many(twins, k)
    for i, (g, t) in enumerate(zip(gang, twins)):
        assert same_state(g, t, f"member {i}: the retried call") == entered[i] + k
    for i, (g, t) in enumerate(zip(gang, twins)):
        g.advance(3)
        t.advance(3)
        same_state(g, t, f"member {i}: three steps alone behind it")
    ea.advance_many(gang, 5)
    ea.advance_many(twins, 5)
    for i, (g, t) in enumerate(zip(gang, twins)):
        assert same_state(g, t, f"member {i}: the gang's next call") == entered[i] + k + 8
    counted[name] = failures


# ---- 7. read-back -------------------------------------------------------------------------------------------------------------------
def read_back_case(ea, H_):
    L = ea._lib()
    for n in (3, 64, 65):
        for method, steps in ((METHOD, 5), (METHOD, STARTUP + 2), (SRKN, 3)):
            g = integration(ea, n, method, steps)
            what = f"n = {n}, {method} after {steps} steps"
            assert H_.fail_alloc(1) == 0                                   # armed and never reached: a read-back allocates nothing
            pos, vel, t, sc = g.state()
            assert sc == steps and t == steps * H and np.isfinite(pos).all() and np.isfinite(vel).all(), what
            p1, v1 = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
            t1, c1 = C.c_double(-1.0), C.c_uint32(77)
            assert L.eph_nbody_get_state(g._h, ea._p(p1), None, C.byref(t1), None) == ea.OK and np.array_equal(p1, pos) and t1.value == t, what
            assert L.eph_nbody_get_state(g._h, None, ea._p(v1), None, C.byref(c1)) == ea.OK and np.array_equal(v1, vel) and c1.value == sc, what
            t1, c1 = C.c_double(-1.0), C.c_uint32(77)
            assert L.eph_nbody_get_state(g._h, None, None, C.byref(t1), C.byref(c1)) == ea.OK and (t1.value, c1.value) == (t, sc), what
            acc = g.acc()
            assert L.eph_nbody_get_acc(g._h, None) == ea.ERR_BAD_ARGUMENT
            assert H_.fail_alloc(0) == 1, what
            if method == METHOD:                                          # the newest level's acceleration is f(its positions)
                assert np.array_equal(acc, ea.accel_eval(pos, g_mu(n))), what
            c = g.clone()
            assert np.array_equal(acc, c.acc()) and np.abs(acc).min() > 0.0, what
    empty = ea.NBodyIntegration(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), 2.5, H, METHOD)
    assert empty.state()[2:] == (2.5, 0) and empty.acc().shape == (0, 3)
    counted["read-back"] = 0


def g_mu(n):
    return random_system(n)[2]


CASES = {"create": lambda ea, H_: (create_case(ea, H_, ""), create_case(ea, H_, DOUBLE)),
         "clone": lambda ea, H_: (clone_case(ea, H_, ""), clone_case(ea, H_, DOUBLE)),
         "first-batch": lambda ea, H_: (first_batch_case(ea, H_, ea.PATH_FAST, "first-batch-fast"),
                                        first_batch_case(ea, H_, ea.PATH_F32_PAIRS, "first-batch-f32")),
         "prop-clone": prop_clone_case,
         "prop-step": lambda ea, H_: (prop_step_fit_case(ea, H_), prop_step_advance_case(ea, H_)),
         "gang-steady": lambda ea, H_: gang_case(ea, H_, "gang-steady", (STARTUP, STARTUP + 1, STARTUP + 2), 7),
         "gang-startup": lambda ea, H_: gang_case(ea, H_, "gang-startup", (0, 0, 0), STARTUP),
         "read-back": read_back_case}


@pytest.mark.parametrize("case", list(CASES))
def test_lifecycle_under_failing_allocations(gpu, case):
    if _dead_children:
        pytest.skip(f"the child of {_dead_children[0]} died: no further child is started")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(ROOT / "tests" / "test_gpu_nbody_lifecycle.py"), case],
                       capture_output=True, text=True, env=dict(os.environ, EPH_AMD_LIBRARY=str(HOOKS_LIB)), cwd=str(ROOT))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _dead_children.append(case)
    assert r.returncode == 0 and f"{case} ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


# ---- the children ----------------------------------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import ephemeris_explorer_amd as ea
    import hooks
    case = sys.argv[1]
    try:
        CASES[case](ea, hooks.load(os.environ["EPH_AMD_LIBRARY"]))          # the countdown is armed in the library the calls go to
        print(f"{case}: allocations {counted}")
        for name, failures in counted.items():
            assert failures == ALLOCATIONS[name], f"{name}: {failures} allocations, {ALLOCATIONS[name]} before"
    except AssertionError as e:
        print(f"{case} FAILED: {str(e)[:1500]}")
        raise
    print(f"{case} ok")
