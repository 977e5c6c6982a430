"""-m gpu: the body-table lookup of the sweep kernels on synthetic tables with planted epochs (tests/synthetic_tables.py, whose docstring
says which kernel arm every scenario is there for), bit for bit against orc.Craft on the oracle's copy of the same parts. The C oracle is
pinned to the Python restatement on the same scenarios by tests/test_synthetic_tables.py; every scenario's liveness predicate is asserted
again here, on the oracle results the device is compared with. No tolerance anywhere: status, attempts, steps, time, state, next_h and
every knot of every craft.

The scenarios run in this process on the wave-per-craft kernel (k_craft_wave: the batches are small) and, one child process per form (the
kernel form is read once per process; this file run as a script), on k_craft_propagate with the craft dealt to the lanes, k_craft_propagate
undealt (craft i on lane i) and k_craft_queue. The direct evaluators -- Solution.eval (k_spline_eval) and SpacecraftBatch.eval with a
reference body (k_craft_eval_reference, and body_state_vector per lane) -- are compared with orc.Solution.eval at the planted epochs.

Not asserted: that the dyadic tables take the shared-reciprocal path. Ephemeris.export_image() is the host's image (start, interval, mu,
counts and rows); the device's rinv is not in it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import synthetic_tables as syn
from conftest import ROOT
from craft_cases import bits, same
from oracle import orc

pytestmark = pytest.mark.gpu

SCENARIOS = {sc.name: sc for sc in syn.scenarios()}
CASES = [(name, m, 0) for name, sc in SCENARIOS.items() for m in sc.methods] + [("A", "Verner87", 4)]
EVAL_SCENARIOS = ["A", "B-inexact", "C", "D-huge-middle", "D-65"]
_oracle_solutions = {}


def oracle_solution(name):
    if name not in _oracle_solutions:
        _oracle_solutions[name] = orc.Solution.from_parts(*SCENARIOS[name].table)
    return _oracle_solutions[name]


def device_run(ea, sc, method, variant=0):
    """the scenario's batch on the product: the table through Solution.from_parts -> Ephemeris, then the call sequence"""
    ea.set_pair_variant(variant)
    try:
        eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
        p = sc.params
        params = ea.AdaptiveParams(p["h_init"], p["h_max"], p["tol_pos"], p["tol_vel"], 1.0 / 5.0, 5.0 / 1.0, 9.0 / 10.0, 1_000_000)
        batch = ea.SpacecraftBatch(eph, sc.t0, sc.pos, sc.vel, method, params, sc.burns, max_knots=sc.max_knots)
    finally:
        ea.set_pair_variant(0)
    if sc.body_order is not None:
        batch.set_body_order(sc.body_order)
    for what, arg in sc.calls:
        if what == "propagate":
            batch.propagate(arg)
        else:
            batch.step_n(arg)
    return batch


def check_scenario(ea, name, method, variant=0):
    sc = SCENARIOS[name]
    orc.set_pair_variant(variant)
    try:
        res = syn.run_oracle(sc, method, oracle_solution(name))
    finally:
        orc.set_pair_variant(0)
    sc.liveness(sc, method, res)
    batch = device_run(ea, sc, method, variant)
    st, gs = batch.status(), batch.state()
    for i, r in enumerate(res):
        what = f"{name} {method} variant {variant} craft {i}"
        cs = r["craft"].state()
        assert st["status"][i] == r["status"], f"{what}: status {st['status'][i]} vs {r['status']}"
        assert st["attempts"][i] == cs["attempts"], f"{what}: attempts {st['attempts'][i]} vs {cs['attempts']}"
        assert st["steps"][i] == cs["steps"], f"{what}: steps {st['steps'][i]} vs {cs['steps']}"
        assert bits(gs["t"][i]) == bits(cs["t"]), f"{what}: time {gs['t'][i]!r} vs {cs['t']!r}"
        ot, op, ov = r["craft"].knots()
        assert st["nknots"][i] == len(ot), f"{what}: {st['nknots'][i]} vs {len(ot)} knots"
        kt, kp, kv = batch.knots(i, st["nknots"][i])
        first = np.flatnonzero((bits(kt) != bits(ot)) | (bits(kp) != bits(op)).any(axis=1) | (bits(kv) != bits(ov)).any(axis=1))
        assert len(first) == 0, f"{what}: knots differ from knot {first[0]} of {len(ot)} on (t = {ot[first[0]]!r})"
        assert same(gs["pos"][i], cs["pos"]) and same(gs["vel"][i], cs["vel"]), f"{what}: state"
        assert bits(gs["next_h"][i]) == bits(cs["next_h"]), f"{what}: next_h {gs['next_h'][i]!r} vs {cs['next_h']!r}"
    return batch, res


@pytest.mark.parametrize("name,method,variant", CASES)
def test_lookup_scenario_on_the_wave_kernel(gpu, name, method, variant):
    check_scenario(gpu, name, method, variant)


@pytest.mark.parametrize("form", ["thread-static", "thread-static-undealt", "thread-queue"])
def test_lookup_scenarios_on_the_other_sweep_kernels(gpu, form):
    """every scenario again on k_craft_propagate (craft dealt to the lanes, and craft i on lane i) and on k_craft_queue"""
    env = dict(os.environ, EPH_CRAFT_FORM="thread", EPH_CRAFT_QUEUE="1" if form == "thread-queue" else "0",
               EPH_CRAFT_SORT="0" if form.endswith("undealt") else "1")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_gpu_craft_lookup.py"), form], env=env, cwd=str(ROOT), capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and f"{form} ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


@pytest.mark.parametrize("name", EVAL_SCENARIOS)
def test_solution_eval_at_the_planted_epochs(gpu, name):
    """k_spline_eval, with and without the velocity: start, every boundary and its two neighbours, start + span and its upper neighbour,
    +-inf of every body"""
    sc = SCENARIOS[name]
    sol, osol = gpu.Solution.from_parts(*sc.table), oracle_solution(name)
    for b in range(sc.n_bodies):
        at = syn.planted_epochs(sc, b)
        pos, vel, inside = sol.eval(b, at)
        pos_only, none, inside_p = sol.eval(b, at, with_velocity=False)
        assert none is None
        for k, t in enumerate(at):
            want, wpos = osol.eval(b, t), osol.eval(b, t, with_velocity=False)
            assert inside[k] == inside_p[k] == (want is not None), f"{name} body {b} at {t!r}: inside {inside[k]}"
            if want is not None:
                assert same(pos[k], want[0]) and same(vel[k], want[1]), f"{name} body {b} at {t!r}: {pos[k]!r} {vel[k]!r} vs {want!r}"
                assert same(pos_only[k], wpos), f"{name} body {b} at {t!r}: position {pos_only[k]!r} vs {wpos!r}"
        assert inside.sum() >= 4


def test_batch_eval_relative_to_a_body_at_the_planted_epochs(gpu):
    """scenario A's batch, whose knots lie on the boundaries of body 0: RelativeTrajectory::state_vector against the 64 s body and the
    256 s body at their planted epochs, the epochs shared (k_craft_eval_reference) and per craft (body_state_vector in every lane)"""
    sc = SCENARIOS["A"]
    batch, res = check_scenario(gpu, "A", "Verner87")
    osol = oracle_solution("A")
    for body in (0, 2):
        at = syn.planted_epochs(sc, body)
        shared = batch.eval(at, reference_body=body)
        own = batch.eval(np.repeat(at[:, None], sc.n, axis=1), reference_body=body)
        hits = 0
        for i in (0, 1, 63, 64, 69):
            kt, kp, kv = res[i]["craft"].knots()
            for k, t in enumerate(at):
                r, h = osol.eval(body, t), orc.hermite_eval(kt, kp, kv, t)
                ok = r is not None and h is not None
                for pos, vel, inside in (shared, own):
                    assert inside[k, i] == ok, f"body {body} craft {i} at {t!r}: inside {inside[k, i]}"
                    if ok:
                        assert same(pos[k, i], h[0] - r[0]) and same(vel[k, i], h[1] - r[1]), f"body {body} craft {i} at {t!r}"
                hits += ok
        assert hits == 5 * np.count_nonzero((at >= 4096.0) & (at <= 5120.0)) >= 5 * 13       # every planted epoch the knots cover


# ---- the child: every scenario on the sweep kernel the environment selects ---------------------------------------------------------
if __name__ == "__main__":
    import ephemeris_explorer_amd as ea
    assert os.environ.get("EPH_CRAFT_FORM") == "thread"
    for case in CASES:
        check_scenario(ea, *case)
    print(f"{sys.argv[1]} ok")
