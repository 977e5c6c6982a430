"""-m gpu: the 4-body, the twelve-wave 8-body and the six-wave 8-body (duo) workgroup forms of csrc/step_wg.hip OFF their fast path,
against the C oracle, bit pattern against bit pattern and nothing else (the scenes and the restated schedule: tests/wg_small_scenes.py;
that every scene reaches the unit, the tile and the branch it names, and stays there through the quiet steps taken here:
tests/test_wg_small_scenes.py; the one-line changes this file was run against: profiles/wg_small_forms.md).

    form   unit of one range test                          launched by
    wg4    wg_pair_tile<1>: one body, one tile             test_forced_accelerations[wg4], test_forced_steps[wg4-*] (k_accel_wg<4>,
                                                             k_lm_step_wg<12 | 13, 4>), test_natural[600-*]
    wg8    wg_pair_tile<1>: one body, tile 0, 1 or a       test_forced_accelerations[wg8] and [duo] (k_accel_wg<8>: launch_accel turns
             last single tile                                wb 9 into 8, so the child for EPH_WG_BODIES=9 runs the TWELVE-wave form
           wg_pair_tile2<1>: one body, two tiles (M = 2)     here), test_forced_steps[wg8-*] (k_lm_step_wg<12 | 13, 8>),
                                                             test_range_ends_of_the_staged_term[wg8], test_natural[1100-*] (accel_eval
                                                             and the start-up)
    duo    wg_pair_tile<2>, wg_pair_tile2<2> (M = 4):      test_forced_steps[duo-*] (k_lm_step_wg<12 | 13, 8, true>: the fused step is
             two bodies, one or two tiles                    the only road to it), test_range_ends_of_the_staged_term[duo],
                                                             test_natural[1100-*] (the fused steps)

EPH_FORCE=wg and EPH_WG_BODIES = 4 | 8 | 9 are read once per process: a child process per form and battery, one at a time; once a
child has failed, been killed or timed out, no later test of this file starts anything on the card. Inside a child the evaluation
order is switched with set_pair_variant on both sides and put back to 0; an order is begun only if the one before it passed.

Two kinds of scene. near, far, massless, tiny_mass and coincident are outside the GUARDED ranges but inside the range where the
wrapper-free sequences are still exact: they hold the slow branch and the code behind it (every term of a failing unit in the IEEE
form, with its own operands, mass and rows, beside fast units in the same launch). far(s, 2^400), faint_tile and thin_tile are
operands the sequences are WRONG for while every result stays finite: they hold the range test itself -- each term of each ballot.

The steps are QUIET: t0 = 0, h = 2^-400, zero initial velocities. At h = 1 / 1024 a near pair's mutual acceleration (about 2^319)
throws it apart in the start-up and the scene fails for every unit like a far one; at 2^-400 the positions keep their planted
operands through L + 3 steps (asserted on the CPU) while the velocities (up to 7e-25) carry the accelerations' bits."""
import os
import subprocess
import sys

import pytest

import wg_small_scenes as wg
from conftest import ROOT
from oracle import orc
from test_gpu_step_phases import PRELUDE

pytestmark = pytest.mark.gpu

FORM_VARIABLES = ("EPH_FORCE", "EPH_WG_BODIES", "EPH_BPW", "EPH_PAIR_VARIANT")

CHILD = r'''
sys.path.insert(0, sys.argv[1] + "/tests")
import wg_small_scenes as wg
form, battery, ks = sys.argv[2], sys.argv[3], [int(k) for k in sys.argv[4].split(",")]
def orders(k):
    ea.set_pair_variant(k)
    orc.set_pair_variant(k)
    orc.set_pair_variant(k, native=True)
def quiet_run(pos, mu, method, what, still=False):
    L = wg.METHODS[method]
    vel = wg.zero_velocities(len(mu))
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, wg.QUIET_H, method)
    o = orc.NBody(pos, vel, mu, 0.0, wg.QUIET_H, method, native=True)
    g.advance(L + 3)
    assert o.advance(L + 3) == 0
    wg.assert_same_run(g, o, f"{form}: {what}, {method}, {L} + 3 quiet steps")
    assert g.state()[3] == L + 3 and np.isfinite(g.state()[1]).all() and np.isfinite(g.acc()).all(), what
    assert (g.acc() != 0.0).any() and (g.state()[1] != 0.0).any() != still, what   # (a still scene: acc() alone carries the bits)
scenes = wg.scenes_330() + ([] if form == "wg4" and battery == "steps" else wg.scenes_280())
for k in ks:                                                # (an order is begun only if the one before it passed)
    orders(k)
    if battery == "accel":
        for sc in scenes:
            wg.assert_same(ea.accel_eval(sc.pos, sc.mu), orc.gravity(sc.pos, sc.mu), f"{form}: accel_eval, {sc.name}, order {k}")
    elif battery == "steps":
        for sc in scenes:
            quiet_run(sc.pos, sc.mu, "QuinlanTremaine12", f"{sc.name}, order {k}", sc.still)
        sc = wg.scene(wg.STORMER)
        quiet_run(sc.pos, sc.mu, "Stormer13", f"{sc.name}, order {k}")
    elif battery == "ends":
        for end, low, pos, mu, band in wg.ends_cases(k):    # (the band conditions are asserted in there, before the comparison)
            what = f"range end 2^{'-' if low else ''}{end}, order {k}, {band} operands in the band"
            a = ea.accel_eval(pos, mu)
            assert np.all(np.isfinite(a)) and np.all(np.abs(a[a != 0]) >= 2.0 ** -1022), f"{form}: a product left the normal range, {what}"
            wg.assert_same(a, orc.gravity(pos, mu), f"{form}: accel_eval, {what}")     # M = 2: wg_pair_tile2<1> (the child for 9 too)
            if form == "duo":                               # M = 4: wg_pair_tile2<2> exists in the fused step only
                quiet_run(pos, mu, "QuinlanTremaine12", what)
orders(0)
print("ok")
'''

_failed = []            # the first child of this module that failed, hung or was killed: no later test starts anything on the card


def child(form, battery, ks, timeout=240):
    assert not _failed, f"not started: an earlier child of this file failed ({_failed[0]})"
    env = {k: v for k, v in os.environ.items() if k not in FORM_VARIABLES}
    env.update(EPH_FORCE="wg", EPH_WG_BODIES=str(wg.FORCED[form]))
    _failed.append(f"{form} {battery} {ks}")                 # (a timeout raises out of subprocess.run: it stays marked)
    r = subprocess.run([sys.executable, "-c", PRELUDE + CHILD, str(ROOT), form, battery, ",".join(map(str, ks))], env=env,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0 or not r.stdout.strip().endswith("ok"):
        said = [line for line in r.stderr.splitlines() if line.startswith("AssertionError")]
        pytest.fail(f"{said[0] if said else f'EPH_WG_BODIES={wg.FORCED[form]} {battery}: the child ended with status {r.returncode}'}\n"
                    f"--- stdout ---\n{r.stdout[-1000:]}\n--- stderr ---\n{r.stderr[-3000:]}", pytrace=False)
    _failed.clear()


@pytest.mark.parametrize("form", list(wg.FORMS))
def test_forced_accelerations(gpu, form):
    """accel_eval on every scene of n = 330 and n = 280 in orders 0, 4, 5 and 6: k_accel_wg<4> and k_accel_wg<8>. The child for
    EPH_WG_BODIES=9 (duo) runs the same through the TWELVE-wave 8-body form: the six-wave form has no k_accel_wg (launch_accel)"""
    child(form, "accel", wg.ORDERS)


@pytest.mark.parametrize("ks", [(0, 4), (5, 6)], ids=["orders-0-4", "orders-5-6"])
@pytest.mark.parametrize("form", list(wg.FORMS))
def test_forced_steps(gpu, form, ks):
    """QuinlanTremaine12, 12 + 3 quiet steps on every scene of n = 330 (and of n = 280 on the big-tile schedule: wg8, duo), and
    Stormer13, 13 + 3, on near(200,11): the planted units inside k_lm_step_wg<L, 4>, <L, 8> and <L, 8, true>. State, time, step
    count and acc() are the oracle's"""
    child(form, "steps", ks)


@pytest.mark.parametrize("form", ["wg8", "duo"])
def test_range_ends_of_the_staged_term(gpu, form):
    """pair_finish_staged at M = 2 (wg8: accel_eval) and M = 4 (duo: stepped quietly) at the ends of the guarded range, as
    test_gpu_step_units.py holds it at M = 5, 4, 3 in the 16-body form: 200 bodies on a jittered 6 x 6 lattice of layers scaled so
    that the smallest n2 lies just above 2^-(end - 1), then the largest just below 2^(end - 1); order 0 at 2^+-300, order 5 at
    2^+-133. Every n2 stays inside the order's guarded range, so every tested unit of the pair {2, 3} stays on the staged sequence"""
    child(form, "ends", (0, 5))


@pytest.fixture(scope="module")
def natural(gpu):
    """the library's own choice of kernel: nothing in the environment forces a form, the evaluation order is 0"""
    forced = [k for k in ("EPH_FORCE", "EPH_WG_BODIES", "EPH_PAIR_VARIANT") if os.environ.get(k)]
    assert not forced, f"{forced} set in the environment: the default dispatch is not what would run"
    assert gpu.pair_variant() == 0
    return gpu


@pytest.mark.parametrize("order", wg.NATURAL_ORDERS)
@pytest.mark.parametrize("n", list(wg.NATURAL_SIZES))
def test_natural(natural, n, order):
    """the kernels as dispatch.cpp chooses them: <4> at 600 bodies; k_accel_wg<8> and k_lm_step_wg<12, 8, true> at 1100. accel_eval
    and 12 + 3 quiet steps on the four scenes of the size, orders 0 and 4"""
    assert not _failed, f"not started: a child of this file failed ({_failed[0]})"
    assert wg.NATURAL_SIZES[n] == ("wg4" if 512 < n <= 1024 else "duo") and 512 < n <= 2048
    def both(k):
        natural.set_pair_variant(k)
        orc.set_pair_variant(k)
        orc.set_pair_variant(k, native=True)
    both(order)
    try:
        for sc in wg.scenes_natural(n):
            wg.assert_same(natural.accel_eval(sc.pos, sc.mu), orc.gravity(sc.pos, sc.mu), f"accel_eval, {sc.name}, order {order}")
            vel = wg.zero_velocities(n)
            g = natural.NBodyIntegration(sc.pos, vel, sc.mu, 0.0, wg.QUIET_H)
            o = orc.NBody(sc.pos, vel, sc.mu, 0.0, wg.QUIET_H, native=True)
            g.advance(12 + 3)
            assert o.advance(12 + 3) == 0
            wg.assert_same_run(g, o, f"{sc.name}, order {order}, 12 + 3 quiet steps")
    finally:
        both(0)
