"""-m gpu: the entry of k_lm_step_wg (csrc/step_wg.hip) in every instantiation. The kernel takes pos_cur, n, lo, hi, npad and cur as
leading plain arguments, which arrive in scalar registers (kernarg preload, a compile flag of step_wg.hip alone in build.py), and
the rest of LmArgs by value behind them; the tail wave of the 16-body form issues its history loads behind its first tile loads.
k_accel_wg is compiled with the same flag, so its entry changes too.

The form is forced per child process (EPH_FORCE=wg with EPH_WG_BODIES = 16, 8, 9 = the six-wave 8-body form, 4: read once per
process). Handles of at most 64 bodies take the workgroup kernels only with set_path(3); such a handle predicts in a launch of its
own at the start of every batch, so the last step of each of its batches is the kernel's `!a.do_predict` arm (a larger unsharded
handle never reaches it). Everything is bit for bit against the CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wg_solout_scenes as ws
from conftest import ROOT
from test_gpu_step_phases import H, PRELUDE, _free_port

pytestmark = pytest.mark.gpu

FORMS = {"wg16": "16", "wg8": "8", "wg8-six-waves": "9", "wg4": "4"}
METHODS = ("QuinlanTremaine12", "Stormer13")                # L = 12 and L = 13

STEPS = r'''
def handles(n, method):
    pos, vel, mu = plummer(n)
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, 1.0 / 1024.0, method)
    g.set_path(3)                                       # the workgroup kernels at n <= 64 as well
    return g, orc.NBody(pos, vel, mu, 0.0, 1.0 / 1024.0, method, native=True)
def agree(g, o, what):
    assert same(g.state()[0], o.state()[0]) and same(g.state()[1], o.state()[1]) and g.state()[2:] == o.state()[2:], what
method, L = sys.argv[2], (13 if sys.argv[2] == "Stormer13" else 12)
'''


def run_form(script, form, *args):
    env = dict(os.environ, EPH_FORCE="wg", EPH_WG_BODIES=FORMS[form])
    env.pop("EPH_PAIR_VARIANT", None)
    r = subprocess.run([sys.executable, "-c", PRELUDE + STEPS + script, str(ROOT), *map(str, args)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("method", METHODS)
def test_sixteen_body_form(gpu, method):
    """k_lm_step_wg<L, 16>: n = 64 (one tile, one interval; the last step of the batch without the predictor), 65 and 128 (two tiles:
    the single-tile phases alone), 300 (five tiles, the last ragged and a late third tile; 12 live bodies in the last workgroup),
    513 (nine tiles, a one-tile last phase; one live body in the last workgroup). Start-up + 7 fused steps."""
    run_form(r'''
for n in (64, 65, 128, 300, 513):
    g, o = handles(n, method)
    g.advance(L + 7)
    assert o.advance(L + 7) == 0
    agree(g, o, ("steps", n, method))
print("ok")
''', "wg16", method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("form", ["wg8", "wg8-six-waves", "wg4"])
def test_small_forms(gpu, form, method):
    """<L, 8> (twelve waves), <L, 8, DUO> (six waves) and <L, 4> (two chain waves) at n = 64 (one tile) and 130 (three tiles, two
    live bodies in the last workgroup): the tail wave of these forms has no tile work and loads its history at its entry, out of
    the preloaded npad and cur"""
    run_form(r'''
for n in (64, 130):
    g, o = handles(n, method)
    g.advance(L + 7)
    assert o.advance(L + 7) == 0
    agree(g, o, ("steps", n, method))
print("ok")
''', form, method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("form", list(FORMS))
def test_every_ring_slot(gpu, form, method):
    """`cur` as a preloaded scalar: 25 = 12 + 13 fused steps behind the start-up, so cur takes every value of 0 .. L - 1 at least
    twice for both L, once as ONE advance(25) (25 launches out of one argument block whose cur changes) and once as 25 single
    advances (25 argument blocks). n = 130; and n = 64, where every single advance is a predict launch (solout.hip:
    k_lm_predict) and a fused step without the predictor."""
    run_form(r'''
for n in (130, 64):
    g, o = handles(n, method)
    one, _ = handles(n, method)
    g.advance(L)
    one.advance(L)
    assert o.advance(L) == 0
    agree(g, o, ("start-up", n, method))
    g.advance(25)
    for k in range(25):
        one.advance(1)
    assert o.advance(25) == 0
    agree(g, o, ("advance(25)", n, method))
    agree(one, o, ("25 x advance(1)", n, method))
print("ok")
''', form, method)


def test_sample_inside_the_batch(gpu, tmp_path):
    """`samp` stays in the by-value block and must reach the tail wave: n = 130 with sampling periods 1, 2, 3, 7 and 12 steps by
    body index, step_n(12) (the start-up), step_n(25) (one fused batch; samples of every period fall due inside it), a take,
    step_n(1), step_n(30), a take: polynomials, spline bounds, times and the final state against the oracle's"""
    sc = ws.Scenario("e130", 130, ops=(("step_n", 12), ("step_n", 25), ("take",), ("step_n", 1), ("step_n", 30), ("take",)))
    npz = tmp_path / "e130.npz"
    np.savez(npz, **ws.run_oracle(sc))
    env = dict(os.environ, EPH_FORCE="wg", EPH_WG_BODIES="16")
    env.pop("EPH_PAIR_VARIANT", None)
    child = r'''
import sys
import numpy as np
root, tests, npz = sys.argv[1:4]
sys.path[:0] = [root, tests]
import ephemeris_explorer_amd as ea
import wg_solout_scenes as ws
sc = ws.Scenario("e130", 130, ops=(("step_n", 12), ("step_n", 25), ("take",), ("step_n", 1), ("step_n", 30), ("take",)))
want = dict(np.load(npz))
assert want["take2_0_npoly"].sum() > 0, "no sample fell due inside the batch"
ws.compare(ws.run(sc, ea.NBodyPropagator), want, "wg16", sc)
print("ok")
'''
    r = subprocess.run([sys.executable, "-c", child, str(ROOT), str(ROOT / "tests"), str(npz)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


def _shard_worker(rank, world, port, n, out):
    sys.path.insert(0, str(ROOT))
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd import parallel
    from ephemeris_explorer_amd.workloads import plummer
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pos, vel, mu = plummer(n)
    if rank == 0:                                          # the single handle, in a process that forces the same kernel
        one = ea.NBodyIntegration(pos, vel, mu, 0.0, H)
        one.advance(12 + 7)
        out["single"] = (one.state(), one.acc())
    # (every rank starts the whole system up, then the partition -- as tests/test_gpu_shard.py does)
    nb = ea.NBodyIntegration(pos, vel, mu, 0.0, H)
    nb.advance(12)
    parallel.shard_nbody(nb, dist, transport="host")
    for k in (3, 1, 3):                                    # three batches: three predict launches, three steps without the predictor
        nb.advance(k)
    out[rank] = (nb.state(), nb.acc(), nb.shard_info())
    dist.barrier()
    dist.destroy_process_group()


def test_target_range_from_the_preloaded_lo_and_hi(gpu, monkeypatch):
    """`lo` / `hi` other than 0 / n: two ranks through the host-staged exchange at n = 712 (768 padded: targets [0, 384) and
    [384, 712)). The second range starts at lo = 384 and ends inside the workgroup of bodies 704-719, so `owner` is tested against
    the preloaded hi there. 12 steps unsharded, then batches of 3, 1 and 3 steps, bit-identical to the single handle's 19."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("EPH_FORCE", "wg")
    monkeypatch.setenv("EPH_WG_BODIES", "16")
    monkeypatch.delenv("EPH_PAIR_VARIANT", raising=False)
    n, world = 712, 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), n, out), nprocs=world, join=True)
    (p0, v0, t0, sc0), a0 = out["single"]
    for r in range(world):
        (p, v, t, sc), a, (lo, hi, gathers) = out[r]
        assert (lo, hi) == (r * 384, min(n, (r + 1) * 384)) and gathers > 0
        assert t == t0 and sc == sc0
        assert np.array_equal(p, p0) and np.array_equal(v, v0) and np.array_equal(a, a0), r


ACCEL = r'''
rng = np.random.default_rng(41)
n = 300
pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
assert same(ea.accel_eval(pos, mu), orc.gravity(pos, mu)), "k_accel_wg, no acc_init"
init = rng.normal(size=(n, 3)) * 1e-9
want = init.copy()                                       # the oracle adds its sum to what ddy holds
orc.lib().orc_newtonian_gravity_eval(n, orc._ptr(np.ascontiguousarray(pos)), orc._ptr(mu), orc._ptr(want))
assert same(ea.accel_eval(pos, mu, init), want), "k_accel_wg, acc_init"
pos, vel, mu = plummer(n)
for method in ("Ruth", "McLachlanO4"):                   # every stage one k_accel_wg launch with the kick and the drift behind it
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, 1.0 / 1024.0, method)
    o = orc.NBody(pos, vel, mu, 0.0, 1.0 / 1024.0, method, native=True)
    g.advance(5)
    assert o.advance(5) == 0
    assert same(g.state()[0], o.state()[0]) and same(g.state()[1], o.state()[1]), ("KickDrift", method)
print("ok")
'''


@pytest.mark.parametrize("form", ["wg16", "wg8", "wg4"])
def test_accel_kernels(gpu, form):
    """k_accel_wg<16>, <8>, <4> at n = 300 (five tiles, the last ragged; the last workgroup partly empty): without and with
    acc_init, and with KickDrift (the symplectic methods' stage launch, which is also the multistep methods' start-up path)"""
    env = dict(os.environ, EPH_FORCE="wg", EPH_WG_BODIES=FORMS[form])
    env.pop("EPH_PAIR_VARIANT", None)
    r = subprocess.run([sys.executable, "-c", PRELUDE + ACCEL, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
