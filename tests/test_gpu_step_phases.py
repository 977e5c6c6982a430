"""-m gpu: the phase schedule of the 16-body workgroup kernel (csrc/step_wg.hip: tiles 0 and 1 singly, then phases of up to three
64-source tiles in two sets of three LDS buffers, pair work dealt by source tile: five bodies against one tile per pair wave).

The kernel is forced (EPH_FORCE=wg EPH_WG_BODIES=16, both read once per process: hence the child processes) at every tile count
from 1 to 12: on both sides of every phase boundary, with last phases of one, two and three tiles, ragged last tiles, the
workgroup's own tile in each position of a phase and body counts that leave the last workgroup partly empty. Everything is bit
for bit against the CPU oracle (O(N^2) on the host: the sizes are small)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
H = 1.0 / 1024.0
FORCED = {"EPH_FORCE": "wg", "EPH_WG_BODIES": "16"}

PRELUDE = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import ephemeris_explorer_amd as ea
from ephemeris_explorer_amd.workloads import plummer
from oracle import orc
same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
'''


def run_forced(script, *args):
    env = dict(os.environ, **FORCED)
    env.pop("EPH_PAIR_VARIANT", None)
    r = subprocess.run([sys.executable, "-c", PRELUDE + script, str(ROOT), *map(str, args)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_accelerations_at_every_tile_count(gpu):
    """tile counts 1..12: phase counts 1, 2, 3 (one, two, three tiles in the last phase), 4, ..., 6; n = 64 k and 64 k + 1 sit on
    the two sides of every tile (and so of every phase) boundary; 17, 641 and 705 leave the last workgroup partly empty"""
    run_forced(r'''
rng = np.random.default_rng(11)
for n in (17, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 576, 577, 641, 705, 768):
    pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
    assert same(ea.accel_eval(pos, mu), orc.gravity(pos, mu)), ("accel", n)
print("ok")
''')


def test_fused_steps_against_the_oracle(gpu):
    """k_lm_step_wg<12, 16> (and <13, 16>: Stormer13) behind the start-up's force evaluations: 12 + 7 steps"""
    run_forced(r'''
for n, method in ((130, "QuinlanTremaine12"), (200, "QuinlanTremaine12"), (330, "QuinlanTremaine12"), (450, "QuinlanTremaine12"),
                  (705, "QuinlanTremaine12"), (330, "Stormer13")):
    pos, vel, mu = plummer(n)
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, 1.0 / 1024.0, method)
    o = orc.NBody(pos, vel, mu, 0.0, 1.0 / 1024.0, method, native=True)
    steps = (13 if method == "Stormer13" else 12) + 7
    g.advance(steps)
    assert o.advance(steps) == 0
    assert same(g.state()[0], o.state()[0]) and same(g.state()[1], o.state()[1]), ("steps", n, method)
print("ok")
''')


def test_slow_path_on_a_five_body_wave(gpu):
    """An operand outside the guarded ranges sends the whole wave (five bodies against one tile) through the IEEE form: bodies 10
    (tile 0) and 100 (tile 1) 2^-160 apart along every axis, so n2 = 3 * 2^-320 is below the guarded range of every order, on a
    tile that is not the workgroup's own; then one massless source (orders 4 and 5 divide mu). Orders 0, 4 and 5."""
    run_forced(r'''
rng = np.random.default_rng(12)
n = 330
for k in (0, 4, 5):
    ea.set_pair_variant(k)
    orc.set_pair_variant(k)
    pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
    close = pos.copy()
    close[10] = 0.0
    close[100] = 2.0 ** -160
    assert same(ea.accel_eval(close, mu), orc.gravity(close, mu)), ("close pair", k)
    massless = mu.copy()
    massless[200] = 0.0
    assert same(ea.accel_eval(pos, massless), orc.gravity(pos, massless)), ("massless source", k)
ea.set_pair_variant(0)
orc.set_pair_variant(0)
print("ok")
''')


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, n, steps, out):
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
        one.advance(12 + steps)
        out["single"] = (one.state(), one.acc())
    # (the host-staged exchange costs ~0.2 s per gather between processes that share a GPU and the start-up has 336 of them:
    # every rank starts the whole system up, then the partition -- as tests/test_gpu_shard.py does)
    nb = ea.NBodyIntegration(pos, vel, mu, 0.0, H)
    nb.advance(12)
    parallel.shard_nbody(nb, dist, transport="host")
    nb.advance(steps)
    out[rank] = (nb.state(), nb.acc(), nb.shard_info())
    dist.barrier()
    dist.destroy_process_group()


def test_target_partition_matches_the_single_handle(gpu, monkeypatch):
    """eph_nbody_shard, two ranks through the host-staged exchange at n = 705 (768 padded: 384 targets per rank, the second
    rank's range starts at tile 6 and ends in a partly empty workgroup), 12 + 7 steps, the workgroup kernel forced in every
    process: bit-identical to the single handle"""
    import torch.multiprocessing as mp
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    n, world, steps = 705, 2, 7
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), n, steps, out), nprocs=world, join=True)
    (p0, v0, t0, sc0), a0 = out["single"]
    for r in range(world):
        (p, v, t, sc), a, (lo, hi, gathers) = out[r]
        assert (lo, hi) == (r * 384, min(n, (r + 1) * 384)) and gathers > 0
        assert t == t0 and sc == sc0
        assert np.array_equal(p, p0) and np.array_equal(v, v0) and np.array_equal(a, a0), r
