"""-m gpu: every writer of the live table either completes or changes nothing (csrc/ephemeris_table.h), and so does
eph_craft_batch_set_body_order.

The allocation-failure paths are run with the test hook eph_debug_fail_alloc(n) (csrc/eph_debug.h): the n-th device allocation the
library makes on this thread returns EPH_ERR_OUT_OF_MEMORY before any HIP call. For n = 1, 2, ... a writer is called until it
succeeds: after every failure the table's image, every body's info and the revision are byte-identical to what they were, and the
countdown has disarmed itself; after the success the table equals one created from the host-joined solution, and the device's rows
give the positions eph_solution_eval gives for that solution, bit for bit. No fault is provoked anywhere: a host function returns an
error code.

Each test is one child process (this file run as a script) with EPH_AMD_LIBRARY naming the test-hooks library, which carries the
hook beside the product's objects."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_system

pytestmark = pytest.mark.gpu
DAY = 86400.0
HOOKS_LIB = ROOT / "ephemeris_explorer_amd" / "libephemeris_amd_testhooks.so"
MAX_K = 8                 # a writer that allocates more often than this allocates inside a loop


def _child(case):
    env = dict(os.environ, EPH_AMD_LIBRARY=str(HOOKS_LIB))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(ROOT / "tests" / "test_gpu_table_commit.py"), case], env=env,
                       cwd=str(ROOT), capture_output=True, text=True)
    assert r.returncode == 0 and f"{case} ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("case", ["append", "prepend", "merge-trims", "clear-front"])
def test_relayout_synthetic(gpu, case):
    """1. three bodies of 2 polynomials; 40 more per body cannot fit max(2, 32) rows of headroom, so the table is laid out afresh:
    append, prepend, a forward merge that trims, and (6 polynomials, no allocation at all) clear_before"""
    _child(case)


def test_within_headroom_real_data(gpu):
    """2. the first piece of test_gpu_live_ephemeris.py's recipe, 4 craft on Verner87 run off its end; the second piece is merged
    under the countdown; the craft resume into the new span like the oracle's"""
    _child("headroom")


def test_body_order_survives_a_failed_change(gpu):
    """3. set_body_order(P2) fails at its first and at its second allocation: the batch goes on with P1, like the oracle"""
    _child("body-order")


# ---- the child ------------------------------------------------------------------------------------------------------------------
def _snapshot(eph):
    return eph.export_image().tobytes(), [eph.info(b) for b in range(eph.n_bodies)], eph.revision


def _until_ok(H, ea, eph, call, what, after_failure=None):
    """call() under fail_alloc(1), (2), ... until EPH_OK, by k = MAX_K at the latest -> that k. After every failure: the table is what
    it was (host-only assertions, before anything launches a kernel) and the hook has disarmed itself."""
    before = _snapshot(eph)
    for k in range(1, MAX_K + 1):
        assert H.fail_alloc(k) == 0
        st = call()
        if st == ea.OK:
            H.fail_alloc(0)
            return k
        assert st == ea.ERR_OUT_OF_MEMORY, f"{what}: k = {k}: status {st}"
        assert b"injected allocation failure" in ea._lib().eph_last_error(), f"{what}: k = {k}"
        now = _snapshot(eph)
        assert now[0] == before[0] and now[1] == before[1] and now[2] == before[2], f"{what}: k = {k}: the table changed"
        assert H.fail_alloc(0) == 0, f"{what}: k = {k}: the countdown is still armed"
        if after_failure:
            after_failure(k)
    raise AssertionError(f"{what}: no EPH_OK by k = {MAX_K}")


def _device_position(ea, eph, body, t):
    """Body `body`'s position at t as the DEVICE table gives it, all 64 bits: eph_plot_points' first point is the source's position
    at the window's start, through the view's `(p - cell) -> f32`. With the identity grid, p - cell is exact once cell is p's leading
    bits, so three calls (cell = 0, then the sum of what came back) return p's 53 bits in three f32 pieces whose f64 sum is p."""
    cell = np.zeros(3)
    for _ in range(3):
        view = dict(camera_position=(0.0, 0.0, 0.0), cell_offset=cell, current=t)
        req = dict(source_body=body, start=t, end=np.inf, tan2_angular_resolution=1e-3, max_points=1)
        (status, _, pt, xyz), = ea.plot_points(eph, view, [req])
        assert status == 0 and len(pt) == 1 and pt[0] == t, (status, pt, t)
        cell = cell + xyz[0].astype(np.float64)
    return cell


def _same_positions(ea, eph, solution, epochs, what):
    for b in range(eph.n_bodies):
        for t in epochs[b]:
            want, _, inside = solution.eval(b, [t])                  # (with the velocity: UniformSpline::state_vector, what the plot evaluates)
            assert inside[0], (what, b, t)
            got = _device_position(ea, eph, b, float(t))
            assert got.tobytes() == want[0].tobytes(), f"{what}: body {b} at {t!r}: {got!r} vs {want[0]!r}"


def _synthetic(ea, rng, first, npoly):
    """three bodies (intervals 128, 256, 512 s: every bound is an integer), body b's polynomials [first, first + npoly) counted from
    t = 0; 2 to 5 coefficient rows each, any finite numbers"""
    iv = np.array([128.0, 256.0, 512.0])
    polys = [[rng.normal(0.0, 1e3, size=(int(rng.integers(2, 6)), 3)) for _ in range(npoly)] for _ in range(3)]
    return ea.Solution.from_parts(iv * first, iv, polys), iv


def child_relayout(ea, H, case):
    rng = np.random.default_rng(20261018)
    L = ea._lib()
    mu = np.array([1.0, 2.0, 3.0])
    n0 = 6 if case == "clear-front" else 2
    base, iv = _synthetic(ea, rng, 0, n0)
    img_of = lambda sol: ea.Ephemeris(sol, mu).export_image().tobytes()                    # noqa: E731
    joined, _ = _synthetic(ea, np.random.default_rng(20261018), 0, n0)                     # the same polynomials, joined on the host
    assert img_of(joined) == img_of(base)
    eph = ea.Ephemeris(base, mu)
    lo, hi = 0, n0                                                                         # the polynomials of the table afterwards
    if case == "append":
        piece, _ = _synthetic(ea, rng, 2, 40)
        call = lambda: L.eph_ephemeris_append(eph._h, piece._h, 1)                         # noqa: E731
        joined.append(piece)
        hi = 42
    elif case == "prepend":
        piece, _ = _synthetic(ea, rng, -40, 40)
        call = lambda: L.eph_ephemeris_append(eph._h, piece._h, -1)                        # noqa: E731
        joined.append(piece, ea.BACKWARD)
        lo = -40
    elif case == "merge-trims":
        piece, _ = _synthetic(ea, rng, 1, 40)                                              # starts where polynomial 1 does: that one goes
        call = lambda: L.eph_ephemeris_merge(eph._h, piece._h, 1)                          # noqa: E731
        for b in range(3):
            joined.clear_after(iv[b] * 1, b)
        joined.append(piece)
        hi = 41
    else:
        at = 2.5 * iv                                                                      # inside polynomial 2: 0, 1 and 2 go (clear_before
        lo = 3                                                                             # drops the polynomial that contains `at` too)
    old_sol, _ = _synthetic(ea, np.random.default_rng(20261018), 0, n0)                    # what the table holds until the writer succeeds
    probe = lambda k: _same_positions(ea, eph, old_sol, [[iv[b] * (n0 - 0.25)] for b in range(3)], f"{case}: after failure {k}")   # noqa: E731
    if case == "clear-front":
        for b in range(3):                                                                 # body by body: three writers
            k = _until_ok(H, ea, eph, lambda: L.eph_ephemeris_clear(eph._h, b, float(at[b]), 0), f"{case} body {b}", probe)
            joined.clear_before(float(at[b]), b)
            assert k == 1, k                                                               # a clear allocates nothing
    else:
        k = _until_ok(H, ea, eph, call, case, probe)
        assert k == 3, k                                                                   # the fresh coefficient and count arrays, nothing else
    for b in range(3):
        assert eph.info(b) == joined.info(b) == (iv[b] * lo, iv[b], hi - lo), (eph.info(b), joined.info(b))
    assert eph.export_image().tobytes() == img_of(joined), f"{case}: image"
    # 8 epochs per body across the old and the new polynomials (the ends included where they are inside)
    epochs = [iv[b] * (lo + (hi - lo) * np.array([0.0, 0.013, 0.11, 0.37, 0.5, 0.77, 0.93, 0.999])) for b in range(3)]
    _same_positions(ea, eph, joined, epochs, case)
    # and the table goes on working: one more append within the new headroom
    more, _ = _synthetic(ea, rng, hi, 3)
    assert _until_ok(H, ea, eph, lambda: L.eph_ephemeris_append(eph._h, more._h, 1), f"{case}: one more") == 1
    joined.append(more)
    assert eph.export_image().tobytes() == img_of(joined)
    _same_positions(ea, eph, joined, [[iv[b] * (hi + 1.5)] for b in range(3)], f"{case}: one more")


def _pieces(ea, orc, s, n):
    count = np.minimum(s.count, 2)
    g = ea.NBodyPropagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, count, s.degree)
    o = orc.Propagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, count, s.degree)
    out = []
    for k in range(1, n + 1):
        t = s.epoch + (1 + 3 * k) * DAY
        g.step_to(t)
        assert o.step_to(t) == 0
        out.append((g.take_solution(), o.take_solution()))
    return out


def child_headroom(ea, H):
    from oracle import orc
    from test_gpu_live_ephemeris import _compare, _fleet, _ship
    s = load_system("simple_solar_system_2433282.5")
    pcs = _pieces(ea, orc, s, 2)
    ship = _ship()
    eph, olive = ea.Ephemeris(pcs[0][0], s.mu), pcs[0][1].clone()
    pos, vel = _fleet(ship, 4, 3)
    batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=8192)
    crafts = [orc.Craft(olive, s.mu, ship.start, pos[i], vel[i], "Verner87") for i in range(4)]
    end = s.epoch + 6.5 * DAY
    batch.propagate(end)
    for i, c in enumerate(crafts):
        assert c.step_to(end) == orc.EVAL_FAILED
        _compare(batch, i, c, ea.EVAL_FAILED, f"craft {i}: first table's end")
    k = _until_ok(H, ea, eph, lambda: ea._lib().eph_ephemeris_merge(eph._h, pcs[1][0]._h, 1), "merge of the second piece")
    print("merge succeeded at k =", k)
    for b in range(s.n):
        olive.clear_after(pcs[1][1].info(b)[0], b)
    assert olive.append(pcs[1][1])
    for b in range(s.n):
        assert eph.info(b) == olive.info(b)
    batch.retry_failed().propagate(end)
    for i, c in enumerate(crafts):
        assert c.step_to(end) == 0
        _compare(batch, i, c, 0, f"craft {i}: resumed in the new span")


def child_body_order(ea, H):
    from oracle import orc
    from test_gpu_live_ephemeris import _compare, _ship
    s = load_system("simple_solar_system_2433282.5")
    (sg, so), = _pieces(ea, orc, s, 1)
    ship = _ship()
    p1 = np.array([3, 0, 4, 1, 2, 9, 8, 7, 6, 5], dtype=np.int32)
    p2 = np.ascontiguousarray(p1[::-1])
    eph = ea.Ephemeris(sg, s.mu)
    batch = ea.SpacecraftBatch(eph, ship.start, [ship.pos], [ship.vel], "Verner87", max_knots=8192).set_body_order(p1)
    c = orc.Craft(so, s.mu, ship.start, ship.pos, ship.vel, "Verner87", body_order=p1)
    t1, t2 = s.epoch + 1.5 * DAY, s.epoch + 3.5 * DAY
    batch.propagate(t1)
    assert c.step_to(t1) == 0
    _compare(batch, 0, c, 0, "order P1, part of the way")
    for nth in (1, 2):
        assert H.fail_alloc(nth) == 0
        st = ea._lib().eph_craft_batch_set_body_order(batch._h, p2.ctypes.data_as(C.POINTER(C.c_int32)))
        assert st == ea.ERR_OUT_OF_MEMORY, (nth, st)
        assert H.fail_alloc(0) == 0, nth
    batch.propagate(t2)
    assert c.step_to(t2) == 0
    _compare(batch, 0, c, 0, "still order P1 after two failed changes")


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT / "tests"))
    import ephemeris_explorer_amd as ea
    import hooks
    assert ea.LIB_PATH == HOOKS_LIB, ea.LIB_PATH
    case = sys.argv[1]
    if case == "headroom":
        child_headroom(ea, hooks.load())
    elif case == "body-order":
        child_body_order(ea, hooks.load())
    else:
        child_relayout(ea, hooks.load(), case)
    print(f"{case} ok")
