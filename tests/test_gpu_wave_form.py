"""-m gpu: the one-wave-per-block force (csrc/step_wave.hip: wave_force<BPW> under k_accel<BPW> and k_lm_step<BPW, L>) at the edges of
its tile walk, against the C oracle, bit pattern against bit pattern (the scenes, the restated walk and range test:
tests/wave_scenes.py; that every scene takes the branch it names: tests/test_wave_scenes.py).

    what                                                        run by
    BPW = 1, runs of one to seven tiles, whole and ragged n     test_default_dispatch_accelerations, test_default_dispatch_steps
    the fallback branch of a pipelined step, BPW = 1            test_planted_scenes, test_planted_scenes_stepped
    BPW = 2, 4, 8 of k_accel and k_lm_step<BPW, 12 | 13>,       test_forced_bodies_per_wave (EPH_FORCE=wave EPH_BPW=..., both read
      ragged last waves, the fallback branch at every BPW,        once per process: a child each, one at a time)
      a non-zero init, the kick-drift epilogue of k_accel
    BPW = 2 and 8 as the library itself chooses them            test_natural_bodies_per_wave (set_path(1) at 2100 and 8200 bodies)

The evaluation order is switched with set_pair_variant on both sides and put back to 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wave_scenes as ws
from conftest import ROOT
from oracle import orc
from test_gpu_step_phases import PRELUDE

pytestmark = pytest.mark.gpu

SIGNS = {"forward": 1.0, "backward": -1.0}


@pytest.fixture(scope="module")
def natural(gpu):
    """the library's own choice of kernel: nothing in the environment forces a form, the evaluation order is 0"""
    forced = [k for k in ("EPH_FORCE", "EPH_BPW", "EPH_PAIR_VARIANT") if os.environ.get(k)]
    assert not forced, f"{forced} set in the environment: the default dispatch is not what would run"
    assert gpu.pair_variant() == 0
    return gpu


class order_set:
    """the evaluation order on the device and on both oracle libraries, 0 again on the way out"""

    def __init__(self, gpu, order):
        self.gpu, self.order = gpu, order

    def __enter__(self):
        self._set(self.order)

    def __exit__(self, *exc):
        self._set(0)

    def _set(self, k):
        self.gpu.set_pair_variant(k)
        orc.set_pair_variant(k)
        orc.set_pair_variant(k, native=True)


# ---- 1. default dispatch: 65-512 bodies take k_accel<1> / k_lm_step<1, L>
@pytest.mark.parametrize("n", ws.TILE_SIZES)
def test_default_dispatch_accelerations(natural, n):
    """whole numbers of tiles (no ragged special, the diagonal tile the last whole one) and their neighbours; runs of up to seven tiles"""
    pos, _, mu = ws.random_system(n)
    ws.assert_same(natural.accel_eval(pos, mu), orc.gravity(pos, mu), f"accel_eval, {n} bodies")


@pytest.mark.parametrize("sign", list(SIGNS))
@pytest.mark.parametrize("method", list(ws.METHODS))
@pytest.mark.parametrize("n", [192, 449, 512])
def test_default_dispatch_steps(natural, n, method, sign):
    """L + 7 steps: the start-up's evaluations (k_accel<1> with the kick-drift epilogue), then seven fused k_lm_step<1, L>"""
    pos, vel, mu = ws.stepped_system(n)
    steps = ws.METHODS[method] + 7
    g = natural.NBodyIntegration(pos, vel, mu, 0.0, SIGNS[sign] * ws.H, method)
    o = orc.NBody(pos, vel, mu, 0.0, SIGNS[sign] * ws.H, method, native=True)
    g.advance(steps)
    assert o.advance(steps) == 0
    ws.assert_same_run(g, o, f"{method}, {n} bodies, {sign}")


# ---- 2. the planted scenes at BPW = 1
@pytest.mark.parametrize("order", ws.ORDERS)
def test_planted_scenes(natural, order):
    """every scene in the order: where the scene is planted for it, steps of the pipelined runs take the fallback branch (in both
    ping-pong phases, on a run's last step and before it, below and above the wave's own tile); where it is not, the same
    operands stay on the fast sequences"""
    with order_set(natural, order):
        for sc in ws.scenes():
            ws.assert_same(natural.accel_eval(sc.pos, sc.mu), orc.gravity(sc.pos, sc.mu), f"{sc.name}, order {order}")


@pytest.mark.parametrize("order", ws.ORDERS)
@pytest.mark.parametrize("name", ws.STEPPED)
def test_planted_scenes_stepped(natural, name, order):
    """QuinlanTremaine12, 12 + 3 steps on a scene: the fallback branch inside k_lm_step<1, 12>"""
    sc, vel = ws.scene(name), ws.velocities()
    with order_set(natural, order):
        g = natural.NBodyIntegration(sc.pos, vel, sc.mu, 0.0, ws.H)
        o = orc.NBody(sc.pos, vel, sc.mu, 0.0, ws.H, native=True)
        g.advance(12 + 3)
        assert o.advance(12 + 3) == 0
        ws.assert_same_run(g, o, f"{name}, order {order}, 12 + 3 steps")


# ---- 3. BPW = 2, 4, 8 forced
CHILD = r'''
sys.path.insert(0, sys.argv[1] + "/tests")
import wave_scenes as ws
bpw = int(sys.argv[2])
def orders(k):
    ea.set_pair_variant(k)
    orc.set_pair_variant(k)
    orc.set_pair_variant(k, native=True)
for n in ws.BPW_SIZES:                                      # the last wave has clamped copies; 705: twelve tiles
    pos, _, mu = ws.random_system(n)
    ws.assert_same(ea.accel_eval(pos, mu), orc.gravity(pos, mu), f"BPW {bpw}: accel_eval, {n} bodies")
for k in ws.ORDERS:                                         # (an order is begun only if the one before it passed)
    orders(k)
    for sc in ws.scenes():
        ws.assert_same(ea.accel_eval(sc.pos, sc.mu), orc.gravity(sc.pos, sc.mu), f"BPW {bpw}: {sc.name}, order {k}")
    for name in ws.STEPPED:                                 # the fallback branch inside k_lm_step<BPW, 12>
        sc, vel = ws.scene(name), ws.velocities()
        g = ea.NBodyIntegration(sc.pos, vel, sc.mu, 0.0, ws.H)
        o = orc.NBody(sc.pos, vel, sc.mu, 0.0, ws.H, native=True)
        g.advance(12 + 3)
        assert o.advance(12 + 3) == 0
        ws.assert_same_run(g, o, f"BPW {bpw}: {name}, order {k}, 12 + 3 steps")
orders(0)
pos, _, mu = ws.random_system(131, 1)                       # a = init + sum: the lower chain continues from the caller's value
init = np.random.default_rng(1).normal(size=(131, 3)) * 1e-9
want = init.copy()
orc.lib().orc_newtonian_gravity_eval(131, orc._ptr(pos), orc._ptr(mu), orc._ptr(want))
ws.assert_same(ea.accel_eval(pos, mu, init), want, f"BPW {bpw}: accel_eval into a non-zero acc, 131 bodies")
for n in (131, 330):                                        # k_lm_step<BPW, 12> and <BPW, 13>, seven steps behind the start-up
    pos, vel, mu = ws.stepped_system(n)
    for method, L in ws.METHODS.items():
        for h in (ws.H, -ws.H):
            g = ea.NBodyIntegration(pos, vel, mu, 0.0, h, method)
            o = orc.NBody(pos, vel, mu, 0.0, h, method, native=True)
            g.advance(L + 7)
            assert o.advance(L + 7) == 0
            ws.assert_same_run(g, o, f"BPW {bpw}: {method}, {n} bodies, h = {h}")
pos, vel, mu = ws.stepped_system(131)                       # an SRKN method: every stage is k_accel<BPW> with its kick-drift epilogue
g = ea.NBodyIntegration(pos, vel, mu, 0.0, ws.H, "BlanesMoan6B")
o = orc.NBody(pos, vel, mu, 0.0, ws.H, "BlanesMoan6B", native=True)
g.advance(5)
assert o.advance(5) == 0
ws.assert_same_run(g, o, f"BPW {bpw}: BlanesMoan6B, 131 bodies")
print("ok")
'''


@pytest.mark.parametrize("bpw", [2, 4, 8])
def test_forced_bodies_per_wave(gpu, bpw):
    """EPH_FORCE=wave EPH_BPW=2 | 4 | 8, a fresh child for each: accel_eval at sizes that are no multiple of 8 (one odd), every scene
    in orders 0, 4, 5 and 6 (two of them stepped as well), accel_eval into a non-zero acc, the fused steps of both ring lengths with both step signs at 131 and
    330 bodies, and an SRKN method's stages at 131 -- all against the oracle"""
    env = dict(os.environ, EPH_FORCE="wave", EPH_BPW=str(bpw))
    env.pop("EPH_PAIR_VARIANT", None)
    r = subprocess.run([sys.executable, "-c", PRELUDE + CHILD, str(ROOT), str(bpw)], env=env, capture_output=True, text=True,
                       timeout=120)
    if r.returncode != 0 or not r.stdout.strip().endswith("ok"):
        said = [line for line in r.stderr.splitlines() if line.startswith("AssertionError")]
        pytest.fail(f"{said[0] if said else f'EPH_BPW={bpw}: the child ended with status {r.returncode}'}\n"
                    f"--- stdout ---\n{r.stdout[-1000:]}\n--- stderr ---\n{r.stderr[-3000:]}", pytrace=False)


# ---- 4. BPW = 2 and 8 as dispatch.cpp chooses them
@pytest.mark.parametrize("n", [2100, 8200])
def test_natural_bodies_per_wave(natural, n):
    """set_path(1) at 2048-4095 bodies is BPW = 2, from 8192 on BPW = 8 (lm_bodies_per_wave); 2100 and 8200 end in a ragged tile (52
    and 8 sources). The oracle would need about a minute through the start-up at 8200, so the witness is the workgroup kernel
    (set_path(3)), an independent walk of the same sums: 12 + 3 steps, state and acc() identical"""
    from ephemeris_explorer_amd.workloads import plummer
    assert n % ws.TILE in (52, 8)
    pos, vel, mu = plummer(n)
    wave = natural.NBodyIntegration(pos, vel, mu, 0.0, ws.H)
    wg = natural.NBodyIntegration(pos, vel, mu, 0.0, ws.H)
    wave.set_path(1)
    wg.set_path(3)
    wave.advance(12 + 3)
    wg.advance(12 + 3)
    ws.assert_same_run(wave, wg, f"{n} bodies: the wave form against the workgroup kernel")
    assert np.isfinite(wave.acc()).all()
