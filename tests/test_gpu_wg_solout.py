"""-m gpu: the solout sample that the tail wave of k_lm_step_wg stores (csrc/step_wg.hip), in every form of the kernel, against the CPU
oracle: polynomials, spline bounds, time(), integrator_time(), step count after every operation and the final state of the scenarios
of tests/wg_solout_scenes.py, bit pattern against bit pattern.

The oracle runs once per scenario in this process (module-scoped fixtures; orc.Propagator(native=True)) and is written to an .npz; the
device runs in child processes, because EPH_FORCE and EPH_WG_BODIES are read once per process: EPH_FORCE=wg with EPH_WG_BODIES = 4
(<L, 4>, split tiles), 8 (<L, 8>, twelve waves), 9 (<L, 8, DUO>, six waves) and 16 (<L, 16>, the phase schedule, whose tail wave carries
pair work). Then with nothing forced at the sizes that dispatch.cpp sends to each form, and on two ranks of a target partition.
profiles/wg_solout_scenes.md: the one-line changes to the tail code that these cases were run against."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import wg_solout_scenes as ws
from conftest import ROOT

pytestmark = pytest.mark.gpu

FORMS = {"wg4": "4", "wg8": "8", "wg8-six-waves": "9", "wg16": "16"}

CHILD = r'''
import sys
import numpy as np
root, tests, name, npz, label, pair = sys.argv[1:7]
sys.path[:0] = [root, tests]
import ephemeris_explorer_amd as ea
import wg_solout_scenes as ws
sc = ws.by_name(name)
want = dict(np.load(npz))
ea.set_pair_variant(int(pair))
got = ws.run(sc, ea.NBodyPropagator, targets=ws.targets_of(want))
ws.compare(got, want, label, sc)
print("ok")
'''


def run_child(sc, npz, label, forced=None, pair=0):
    env = dict(os.environ)
    for k in ("EPH_FORCE", "EPH_WG_BODIES", "EPH_PAIR_VARIANT"):
        env.pop(k, None)
    if forced is not None:
        env.update(EPH_FORCE="wg", EPH_WG_BODIES=forced)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(ROOT / "tests"), sc.name, str(npz), label, str(pair)], env=env,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or not r.stdout.strip().endswith("ok"):
        # the child's own message first and whole (form, scenario, operation, body): an assert's tuple would be cut in the middle
        said = [line for line in r.stderr.splitlines() if line.startswith("AssertionError")]
        pytest.fail(f"{said[0] if said else f'{label} {sc.name}: the child ended with status {r.returncode}'}\n"
                    f"--- stdout ---\n{r.stdout[-1000:]}\n--- stderr ---\n{r.stderr[-3000:]}", pytrace=False)


def _record(tmp, sc, **kw):
    path = tmp / f"{sc.name}-pv{kw.get('pair_variant', 0)}.npz"
    np.savez(path, **ws.run_oracle(sc, **kw))
    return path


@pytest.fixture(scope="module")
def oracle_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wg_solout")


@pytest.fixture(scope="module")
def oracle(oracle_dir):
    """the oracle's run of every forced scenario, once: {name: path of the .npz}"""
    return {sc.name: _record(oracle_dir, sc) for sc in ws.SCENES}


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
@pytest.mark.parametrize("form", list(FORMS))
def test_forced_form_against_the_oracle(gpu, oracle, form, sc):
    run_child(sc, oracle[sc.name], form, forced=FORMS[form])


@pytest.mark.parametrize("pair", [0, 4])
def test_phase_schedule_under_pair_orders(gpu, oracle_dir, pair):
    """<L, 16>: the tail wave's shed bodies go through the pair wave's code, and evaluation order 4 has a pair wave of its own
    (wg_pair_wave_big): the history registers live across both"""
    sc = ws.by_name("p705")
    run_child(sc, _record(oracle_dir, sc, pair_variant=pair), f"wg16-pair-order-{pair}", forced="16", pair=pair)


@pytest.mark.parametrize("sc", ws.DISPATCH, ids=lambda s: s.name)
def test_default_dispatch_against_the_oracle(gpu, oracle_dir, sc):
    """nothing forced: 530 bodies take <L, 4>, 1030 the six-wave form, 2100 <L, 16> -- the kernels as shipped (the oracle's 2100-body
    sums on 16 threads: same bits)"""
    run_child(sc, _record(oracle_dir, sc, threads=16 if sc.n > 2048 else 1), "default-dispatch")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, name, out):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import ephemeris_explorer_amd as ea
    import wg_solout_scenes as scenes
    from ephemeris_explorer_amd import parallel
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sc = scenes.by_name(name)
    info = []

    class Sharding:
        """the propagator, sharded between the scenario's first and second operation (every rank starts the whole system up: the
        host-staged exchange costs ~0.2 s per gather between processes that share a device, and the start-up has 336 of them)"""

        def __init__(self, *a):
            self.p, self.calls = ea.NBodyPropagator(*a), 0

        def step_n(self, k):
            if self.calls == 1:
                parallel.shard_nbody(self.p, dist, transport="host")
            self.calls += 1
            self.p.step_n(k)
            info.append(self.p.integration().shard_info())

        def __getattr__(self, name):
            return getattr(self.p, name)

    out[rank] = (scenes.run(sc, Sharding), info)
    dist.barrier()
    dist.destroy_process_group()


def test_target_partition_against_the_oracle(gpu, oracle_dir, monkeypatch):
    """two ranks on one device through the host-staged exchange, <L, 16> forced, n = 705 (768 padded: rank 1's targets start at tile 6
    and end in the workgroup that owns one body): step_n(12) unsharded, shard, step_n(70), step_n(1), step_n(13). A sharded handle
    predicts at the start of a batch, so the last step of each of these batches is the kernel's `!a.do_predict` arm (no other
    case reaches it), and the take at step 96 has fitted the samples those steps stored. Every rank samples and fits the bodies
    it owns and gathers the rest: EVERY rank's whole solution is the oracle's, all 705 bodies"""
    import torch.multiprocessing as mp
    monkeypatch.setenv("EPH_FORCE", "wg")
    monkeypatch.setenv("EPH_WG_BODIES", "16")
    monkeypatch.delenv("EPH_PAIR_VARIANT", raising=False)
    monkeypatch.setenv("EPH_PEER_TIMEOUT_MS", "5000")
    sc, world = ws.SHARD, 2
    want = dict(np.load(_record(oracle_dir, sc)))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), sc.name, out), nprocs=world, join=True)
    assert set(out.keys()) == set(range(world))
    for r in range(world):
        got, info = out[r]
        (lo0, hi0, g0), (lo, hi, gathers) = info[0], info[-1]
        assert len(info) == 4 and g0 == 0 and (lo, hi) == (r * 384, min(sc.n, (r + 1) * 384)) and gathers > 0, (r, info)
        ws.compare(got, want, f"wg16-rank-{r}-of-{world}", sc)
        npoly = got[f"take{len(sc.ops) - 1}_0_npoly"]
        assert npoly[:384].sum() > 0 and npoly[384:].sum() > 0                  # polynomials of both ranks' bodies
