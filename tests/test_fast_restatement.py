"""The slice-order restatement of EPH_PATH_FAST's sums (csrc/fast.hip), three times: oracle/eph_oracle.c (orc_set_gravity_slices),
oracle/pyoracle.py (gravity_sliced, Problem.set_gravity_slices) and numpy (tests/fast_restatement.py). Written separately, they must
agree bit for bit before tests/test_gpu_fast_reference.py holds the device to them. No GPU here."""
import numpy as np
import pytest

import fast_restatement as fr
from ephemeris_explorer_amd.workloads import plummer
from oracle import orc, pyoracle as po

H = 1.0 / 1024.0
ORDERS = range(7)


@pytest.fixture(autouse=True)
def _switches_off():
    yield
    orc.set_pair_variant(0)
    po.set_pair_variant(0)
    orc.set_gravity_slices(0, 0)


def _two_body_systems():
    rng = np.random.default_rng(3)
    out = [(rng.normal(size=(2, 3)), rng.uniform(0.5, 2.0, 2)) for _ in range(40)]
    e = np.array([1.0, -0.75, 0.5])
    out.append((np.array([[0.0, 0.0, 0.0], 2.0 ** 151 * e]), np.array([1.0, 2.0 ** -30])))     # n2 above every order's guarded range
    out.append((np.array([[0.1, 0.2, 0.3], 2.0 ** 70 * e]), np.array([1.0, 2.0 ** -30])))      # out of range for orders 4-6 only
    out.append((rng.normal(size=(2, 3)), np.array([0.0, 1.5])))                                # a massless body
    out.append((rng.normal(size=(2, 3)), np.array([2.0 ** -210, 1.5])))                        # mu below the divisions' range
    out.append((np.array([[0.3, -0.2, 0.0], [-0.5, 0.7, 0.0]]), np.array([1.0, 0.0])))         # planar: a zero component, +-0 terms
    out.append((np.array([[0.3, 0.0, 0.0], [-0.5, 0.0, 0.0]]), np.array([0.75, 1.25])))        # two zero components
    return out


@pytest.mark.parametrize("k", ORDERS)
def test_numpy_term_equals_the_oracle_on_two_body_systems(k):
    orc.set_pair_variant(k)
    for pos, mu in _two_body_systems():
        a = orc.gravity(pos, mu)
        assert np.isfinite(a).all()
        assert fr.same_bits(fr.ordered_pair(pos, mu, k), a), (k, pos, mu)           # signs of zeros included
        assert fr.same_bits(fr.ordered_pair(pos[::-1], mu[::-1], k), orc.gravity(pos[::-1], mu[::-1]))


@pytest.mark.parametrize("n", [65, 130])
def test_the_three_sliced_sums_are_bit_equal(n):
    pos, _, mu = plummer(n)
    pos[n // 2, 2] = pos[3, 2]                     # one exactly zero component among the pairs
    mu[7] = 0.0
    y = [po.Vec(*map(float, r)) for r in pos]
    differs = 0
    for S, slice_len in ((64, 4), (12, 12)):       # half of the slices empty at 65, a last slice ragged against n at both
        for k in ORDERS:
            orc.set_pair_variant(k)
            po.set_pair_variant(k)
            ordered = orc.gravity(pos, mu)
            with orc.gravity_slices(S, slice_len):
                c = orc.gravity(pos, mu)
            assert fr.same_bits(orc.gravity(pos, mu), ordered)                      # off again: the reference's order
            p = np.array(po.gravity_sliced(y, list(map(float, mu)), 0.0, S, slice_len))
            v = fr.sliced_gravity(pos, mu, S, slice_len, k)
            assert fr.same_bits(c, p) and fr.same_bits(c, v), (n, S, slice_len, k)
            assert np.abs(c - ordered).max() < 1e-12 * np.abs(ordered).max()
            differs += not fr.same_bits(c, ordered)
    assert differs == 14                           # the switch does something: never the ordered sum's bits at these sizes


def test_slices_that_do_not_cover_the_sources_drop_them():
    """the restatement takes (S, slice_len) literally, as the kernel does: what lies behind S * slice_len is not summed"""
    pos, _, mu = plummer(65)
    with orc.gravity_slices(4, 8):
        c = orc.gravity(pos, mu)
    assert fr.same_bits(c, fr.sliced_gravity(pos, mu, 4, 8))
    with orc.gravity_slices(1, 32):
        head = orc.gravity(pos[:32], mu[:32])
    assert np.abs(c[:32] - head).max() < 1e-12 * np.abs(head).max()


def test_multistep_with_the_switch_set_after_the_start_up():
    """orc.NBody and pyoracle's LinearMultistep2 (QuinlanTremaine12), start-up in the reference's order, then 5 sliced steps"""
    n, S, slice_len = 65, 64, 4
    pos, vel, mu = plummer(n)
    o = orc.NBody(pos, vel, mu, 0.0, H)
    ordered = orc.NBody(pos, vel, mu, 0.0, H)
    prob = po.Problem(pos, vel, mu, 0.0)
    lm = po.LinearMultistep2("QuinlanTremaine12", H, prob)
    assert o.advance(12) == 0 and ordered.advance(12 + 5) == 0
    for _ in range(12):
        assert lm.advance() == 0
    assert fr.same_bits(o.state()[0], np.array(prob.y))
    prob.set_gravity_slices(S, slice_len)
    with orc.gravity_slices(S, slice_len):
        for step in range(5):
            assert o.advance(1) == 0 and lm.advance() == 0
            p, v, t, sc = o.state()
            assert fr.same_bits(p, np.array(prob.y)) and fr.same_bits(v, np.array(prob.dy)), step
            assert fr.same_bits(o.acc(), np.array(lm.cur_a)) and t == prob.time and sc == lm.step_count()
            assert fr.same_bits(o.acc(), fr.sliced_gravity(p, mu, S, slice_len))    # the acceleration of the returned position
    # (5 steps of h = 2^-10 on: the positions may still round to the same doubles; the accelerations do not)
    assert not fr.same_bits(o.acc(), ordered.acc())
    assert np.abs(o.state()[0] - ordered.state()[0]).max() < 1e-12


def test_high_precision_reference_and_derived_bounds_on_the_cpu():
    """What tests/test_gpu_fast_reference.py asks of paths 5 and 6, asked of the CPU: the IEEE sliced sum and a binary32 emulation of
    the f32 loop sit far inside K u sum|c| (they must: the bounds count every rounding at its worst), and every single term is more
    than 8 bounds large, so a bound of this size still notices one source dropped or doubled."""
    for n, S, slice_len in ((65, 64, 4), (130, 64, 4), (705, 64, 12)):
        pos, _, mu = plummer(n)
        a_ref, absum, c = fr.exact_sums(pos, mu)
        bound = (20 + slice_len + S) * fr.U64 * absum
        err = np.abs(fr.sliced_gravity(pos, mu, S, slice_len).astype(np.longdouble) - a_ref)
        assert (err <= bound).all() and float((err / (fr.U64 * absum)).max()) < 10.0
        assert fr.sensitivity_margin(c, bound) > 8.0
        dropped = fr.sliced_gravity(np.delete(pos, n - 2, 0), np.delete(mu, n - 2), S, slice_len)
        assert not (np.abs(dropped.astype(np.longdouble) - np.delete(a_ref, n - 2, 0)) <= np.delete(bound, n - 2, 0)).all()
    for n, S, slice_len in ((65, 64, 32), (130, 64, 32)):
        pos, _, mu = fr.jittered_lattice(n)
        p32, m32 = pos.astype(np.float32), mu.astype(np.float32)
        assert len(np.unique(p32, axis=0)) == n
        a_ref, absum, c = fr.exact_sums(p32, m32)
        bound = (20 + 16 + 1) * fr.U32 * absum
        err = np.abs(fr.f32_emulation(pos, mu, S, slice_len).astype(np.longdouble) - a_ref)
        assert (err <= bound).all() and float((err / (fr.U32 * absum)).max()) < 6.0
        assert fr.sensitivity_margin(c, bound) > 8.0
