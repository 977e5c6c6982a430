"""CPU: the scenes of tests/startup_scenes.py still step on what they were planted for -- checked on the C oracle alone -- and the
restatement of the host's dry run of the time tests (NBodyIntegration::startup_small_steps) agrees with the oracle's statuses. What
the device computes on them is in tests/test_gpu_startup_small.py."""
import numpy as np
import pytest

import startup_scenes as ss
from oracle import orc


def test_status_values_are_the_oracles():
    tiny = ss.bound_scenes()[2][0].make(orc.NBody, "QuinlanTremaine12")
    assert tiny.advance(1) == ss.STEP_SIZE_UNDERFLOW
    bounded = ss.sphere(3).make(orc.NBody, "QuinlanTremaine12")
    bounded.set_bound(0.0)
    assert bounded.advance(1) == ss.BOUND_REACHED


def test_the_bound_lies_strictly_between_two_substep_times_of_macro_step_5():
    (inside, _), (boundary, _), _ = ss.bound_scenes()
    ts = ss.substep_times(inside.t0, inside.h, ss.BOUND_MACRO_STEP)
    first = (ss.BOUND_MACRO_STEP - 1) * ss.SUBSTEPS
    assert ts[first + 1] < inside.bound < ts[first + 2] and ts[first + 1] != ts[first + 2]
    assert boundary.bound == ts[ss.BOUND_MACRO_STEP * ss.SUBSTEPS]
    for method in ss.METHODS:
        o = inside.make(orc.NBody, method)
        assert o.advance(ss.BOUND_MACRO_STEP - 1) == 0
        assert o.advance(1) == ss.BOUND_REACHED                # on the third substep: two were taken
        _, _, t, count = o.state()
        assert t == ts[first + 2] and count == ss.BOUND_MACRO_STEP - 1
        assert o.advance(1) == ss.BOUND_REACHED and o.state()[2] == t
        o = boundary.make(orc.NBody, method)
        assert o.advance(ss.BOUND_MACRO_STEP) == 0 and o.state()[2] == boundary.bound
        assert o.advance(1) == ss.BOUND_REACHED and o.state()[3] == ss.BOUND_MACRO_STEP


def test_the_massless_bodies_are_massless_and_the_masses_distinct():
    massless = [s for s in ss.scenes() if "massless" in s.name]
    assert len(massless) == 2
    for s in massless:
        assert s.mu[s.n // 2] == 0.0 and (np.delete(s.mu, s.n // 2) > 0.0).all()
    for s in ss.scenes():
        if s.name.startswith("plummer") and "massless" not in s.name:
            assert len(set(s.mu)) == s.n and (s.mu > 0.0).all()
    assert any(s.h < 0 for s in ss.scenes()) and any(s.h > 0 for s in ss.scenes())
    assert sorted({s.n for s in ss.scenes()}) == sorted(set(ss.SIZES) | set(ss.SHIPPED.values()))


@pytest.mark.parametrize("method", list(ss.METHODS))
def test_the_plan_enters_the_ring_off_its_initial_slot(method):
    """calls two and three are start-up launches (m = 4 and L - 5) that enter at slots L - 1 and L - 5; the third call's steady
    batch follows its partial start-up; the fourth is steady"""
    L, taken, entries = ss.METHODS[method], 0, []
    for k in ss.plan(L):
        m, _ = ss.dry_run(0.0, ss.H, ss.INF, taken * ss.SUBSTEPS, L, k)
        entries.append((ss.entry_slot(taken, L), m, k - m))
        taken += k
    assert entries == [(0, 1, 0), (L - 1, 4, 0), (L - 5, L - 5, 5), (ss.entry_slot(L + 5, L), 0, 2 * L + 5)]
    o = ss.sphere(32).make(orc.NBody, method)
    assert o.advance(L) == 0 and o.eval_count() == ss.startup_evals(L) == {12: 302, 13: 327}[L]


@pytest.mark.parametrize("method", list(ss.METHODS))
def test_the_dry_run_agrees_with_the_oracle(method):
    """over every scene and the plan: the dry run answers m > 0 exactly where the oracle takes those m macro steps without a
    status, and then ends at the oracle's time"""
    L = ss.METHODS[method]
    cases = [(s, 0) for s in ss.scenes()] + ss.bound_scenes()
    fired = set()
    for scene, _ in cases:
        o = scene.make(orc.NBody, method)
        bound = ss.INF if scene.bound is None else scene.bound
        substeps = 0                                           # of the start-up, as the host counts them
        for k in ss.plan(L):
            t = o.state()[2]
            m, t_after = ss.dry_run(t, scene.h, bound, substeps, L, k)
            want = min(k, L - substeps // ss.SUBSTEPS) if substeps % ss.SUBSTEPS == 0 and substeps // ss.SUBSTEPS < L else 0
            if want:
                probe = o.clone()
                st = probe.advance(want)
                assert (m == want) == (st == 0), (scene.name, k, m, want, st)
                if m:
                    assert probe.state()[2] == t_after, (scene.name, k)
            else:
                assert m == 0
            st = o.advance(k)
            if st:
                fired.add((scene.name, st))
            # the substeps the reference has taken: whole macro steps, and the part of an abandoned one (time tells)
            count = o.state()[3]
            if count < L:
                ts = ss.substep_times(scene.t0, scene.h, count + 1)
                now = o.state()[2]
                part = [i for i in range(ss.SUBSTEPS + 1) if ts[count * ss.SUBSTEPS + i] == now]
                substeps = count * ss.SUBSTEPS + (part[0] if part else 0)
            else:
                substeps = L * ss.SUBSTEPS
    assert fired == {(s.name, what) for s, what in ss.bound_scenes()}


def test_the_library_holds_the_start_up_kernels_of_every_order(product_lib):
    """k_lm_startup_small<SrknPlain | SrknDouble, false> and the gang form <SrknPlain, true>, once per evaluation order of the
    point-mass term, in the product's code object and among its (local) symbols"""
    import subprocess
    assert b"k_lm_startup_small" in product_lib.LIB_PATH.read_bytes()
    symbols = subprocess.check_output(["nm", "--defined-only", str(product_lib.LIB_PATH)]).decode().split()
    kernel = "k_lm_startup_small"
    for k in range(7):
        for state, many in (("9SrknPlain", "0"), ("10SrknDouble", "0"), ("9SrknPlain", "1")):
            mangled = f"3pv{k}{len(kernel)}{kernel}INS0_{state}ELb{many}EEE"
            assert any(mangled in s for s in symbols), (k, state, many)
