"""-m gpu: the spacecraft sweep partitioned over ranks by estimated cost (parallel.balanced_partition, parallel.sharded_sweep).
What a rank computes for a craft does not depend on which other craft share its batch, so the records of the per-rank batches,
scattered back through the partition's index blocks, are the summary of ONE batch of all the craft byte for byte -- t, pos, vel,
next_h, status, nknots, attempts, steps -- and so are a craft's knots. No tolerance anywhere.

First with the ranks played one after another in this process (any world size, an empty block, and one case in which the blocks
and the whole batch run different kernel forms); then two real ranks (two processes sharing the one device, gloo) through the one
call, sharded_sweep, against the table rank 0 built and broadcast."""
import os
import socket

import numpy as np
import pytest

from conftest import ROOT, SYSTEMS, load_system

pytestmark = pytest.mark.gpu
DAY = 86400.0
MAX_KNOTS = 464                                     # (a low orbit writes about 215 knots a day)
SYSTEM = "full_solar_system_2433282.5"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scene(ea):
    from ephemeris_explorer_amd.systems import load_ship
    s = load_system(SYSTEM)
    ship = load_ship(SYSTEMS / SYSTEM / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(s.epoch + 41.0 * DAY)
    return s, ship, sol, ea.Ephemeris(sol, s.mu)


@pytest.fixture(scope="module")
def scene(gpu):
    return _scene(gpu)


def _whole(ea, eph, ship, pos, vel):
    b = ea.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=MAX_KNOTS)
    b.propagate(ship.start + DAY)
    return b, b.summary()


@pytest.mark.parametrize("n,world", [(100, 8), (100, 3), (1, 2), (12290, 2)])
def test_virtual_ranks_reproduce_the_single_batch(gpu, scene, n, world):
    """Blocked mixed population, 1 day. Every block of the balanced partition run as a batch of its own, one after the other;
    their records scattered back through `blocks` equal the summary of one batch of all n craft, and every craft's knots read from
    its block's batch equal those read from the whole batch (12290: every 211th craft and the ends of each block).
    (100, 8): 12 or 13 craft per rank; (100, 3): unequal thirds; (1, 2): one block is empty -- an empty batch, propagated and
    summarised like any other. Up to 12 288 craft a batch runs one wave per craft, so in these three cases blocks and whole batch
    are all in that form; (12290, 2) is the smallest shape at which they differ: the whole batch one thread per craft, dealt to
    the lanes, its two blocks of 6145 one wave per craft."""
    from ephemeris_explorer_amd.parallel import balanced_partition, craft_cost_estimate
    from ephemeris_explorer_amd.workloads import craft_population
    s, ship, _, eph = scene
    pos, vel, _ = craft_population("mixed", n, s, ship, order="blocked")
    blocks = balanced_partition(craft_cost_estimate(s.mu, s.pos, s.vel, pos, vel, DAY), world)
    assert sorted(np.concatenate(blocks).tolist()) == list(range(n))
    whole, want = _whole(gpu, eph, ship, pos, vel)
    assert (want["status"] == 0).all() and (want["t"] >= ship.start + DAY).all()
    got = np.zeros(n, dtype=gpu.SpacecraftBatch.RECORD)
    got["status"] = -99                                            # (an entry no block fills stays visible)
    attempts = []
    for block in blocks:
        b = gpu.SpacecraftBatch(eph, ship.start, pos[block], vel[block], "Verner87", max_knots=MAX_KNOTS)
        assert b.n == len(block)
        b.propagate(ship.start + DAY)
        rec = b.summary()
        assert rec.shape == (len(block),)
        got[block] = rec
        attempts.append(int(rec["attempts"].sum(dtype=np.int64)))
        local = range(len(block)) if n <= 100 else sorted(set(range(0, len(block), 211)) | {len(block) - 1})
        for j in local:
            i = int(block[j])
            mine, theirs = b.knots(j, rec["nknots"][j]), whole.knots(i, want["nknots"][i])
            assert rec["nknots"][j] == want["nknots"][i] >= 2
            for x, y, what in zip(mine, theirs, ("epochs", "positions", "velocities")):
                assert x.tobytes() == y.tobytes(), f"craft {i} (entry {j} of its block): knot {what}"
    for field in got.dtype.names:
        assert got[field].tobytes() == want[field].tobytes(), field
    assert got.tobytes() == want.tobytes()
    if n >= 100:
        a = np.array(attempts, dtype=np.float64)
        print(f"\nn={n} world={world}: per-rank attempts {attempts}, max/mean {a.max() / a.mean():.4f}")


def _worker(rank, world, port, n, out):
    import sys
    sys.path.insert(0, str(ROOT))
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd import parallel
    from ephemeris_explorer_amd.systems import load_ship
    from ephemeris_explorer_amd.workloads import craft_population
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = load_system(SYSTEM)
    ship = load_ship(SYSTEMS / SYSTEM / "ships" / "Mars Transfer Ship.json")
    solutions = []

    def build():                                                   # rank 0 only: the other rank imports the image, and has no Solution
        solutions.append(ea.NBodyPropagator.from_system(s).propagate(s.epoch + 41.0 * DAY))
        return ea.Ephemeris(solutions[0], s.mu)

    eph, _ = parallel.broadcast_ephemeris(build, dist)
    assert len(solutions) == (1 if rank == 0 else 0)
    bodies = parallel.body_states_at(solutions[0] if rank == 0 else None, ship.start, dist)
    pos, vel, _ = craft_population("mixed", n, s, ship, order="blocked")
    kw = dict(mu=s.mu, body_states=bodies, max_knots=MAX_KNOTS, dist=dist)
    res = parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY, **kw)
    assert res["batch"].n == len(res["blocks"][rank])
    own = res["batch"].summary()                                   # the resident batch is this rank's block, in block order
    assert own.tobytes() == res["records"][res["blocks"][rank]].tobytes()
    cont = parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY, partition="contiguous", **kw)
    # a caller that sweeps repeatedly: the previous sweep's attempts as the cost, no estimate
    again = parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY, cost=res["records"]["attempts"], max_knots=MAX_KNOTS,
                                   dist=dist)
    keep = ("records", "blocks", "rank_attempts", "balance", "estimate_s", "partition_s", "sweep_s", "gather_s")
    out[rank] = ({k: res[k] for k in keep}, {k: cont[k] for k in keep}, {k: again[k] for k in keep}, bodies)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sharing_the_device(gpu, scene):
    """sharded_sweep on two ranks (two processes on the one device, gloo): 511 blocked mixed craft for 1 day, blocks of 256 and 255.
    `records` identical on both ranks and byte-equal to the summary of one batch of all 511; max / mean of the per-rank attempts
    <= 1.05 (the review's criterion); partition="contiguous" returns the same records with a larger ratio (printed)."""
    import torch.multiprocessing as mp
    from ephemeris_explorer_amd.parallel import shard_range
    from ephemeris_explorer_amd.workloads import craft_population
    n, world = 511, 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), n, out), nprocs=world, join=True)
    assert set(out.keys()) == {0, 1}
    s, ship, sol, eph = scene
    pos, vel, _ = craft_population("mixed", n, s, ship, order="blocked")
    _, want = _whole(gpu, eph, ship, pos, vel)
    assert (want["status"] == 0).all()
    for r in range(world):
        res, cont, again, bodies = out[r]
        for got, what in ((res, "balanced"), (cont, "contiguous"), (again, "balanced by the last sweep's attempts")):
            assert got["records"].dtype == want.dtype and got["records"].tobytes() == want.tobytes(), (r, what)
            assert len(got["blocks"]) == world and sorted(len(b) for b in got["blocks"]) == [255, 256]
            assert np.array_equal(got["rank_attempts"], [int(want["attempts"][b].sum(dtype=np.int64)) for b in got["blocks"]])
            assert got["balance"] == got["rank_attempts"].max() / got["rank_attempts"].mean()
            assert all(got[k] >= 0.0 for k in ("estimate_s", "partition_s", "sweep_s", "gather_s"))
        assert all(np.array_equal(a, b) for a, b in zip(res["blocks"], out[0][0]["blocks"]))        # the same partition on every rank
        assert [tuple(b[[0, -1]]) for b in cont["blocks"]] == [(lo, hi - 1) for lo, hi in (shard_range(n, q, world) for q in range(world))]
        print(f"\nrank {r}: max/mean attempts balanced {res['balance']:.4f} (by attempts {again['balance']:.4f}), contiguous "
              f"{cont['balance']:.4f}; estimate {res['estimate_s'] * 1e3:.2f} ms, partition {res['partition_s'] * 1e3:.2f} ms, sweep "
              f"{res['sweep_s'] * 1e3:.1f} ms, gather {res['gather_s'] * 1e3:.2f} ms")
        assert res["balance"] <= 1.05
        assert again["balance"] <= 1.05
        assert cont["balance"] > res["balance"]
        # the bodies at the sweep's start, evaluated from rank 0's Solution, reached both ranks; they are the system's own state
        assert np.array_equal(bodies[0], out[0][3][0]) and np.array_equal(bodies[1], out[0][3][1])
        assert bodies[0].shape == (s.n, 3) and np.abs(bodies[0] - s.pos).max() < 1.0 and np.abs(bodies[1] - s.vel).max() < 1e-2


def test_single_process_sharded_sweep(gpu, scene):
    """no process group: one block, the same records, and the argument errors"""
    from ephemeris_explorer_amd import parallel
    from ephemeris_explorer_amd.workloads import craft_population
    s, ship, sol, eph = scene
    n = 24
    pos, vel, _ = craft_population("mixed", n, s, ship, order="blocked")
    bodies = parallel.body_states_at(sol, ship.start)
    res = parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY, mu=s.mu, body_states=bodies, max_knots=MAX_KNOTS)
    _, want = _whole(gpu, eph, ship, pos, vel)
    assert res["records"].tobytes() == want.tobytes() and res["balance"] == 1.0
    assert len(res["blocks"]) == 1 and np.array_equal(res["blocks"][0], np.arange(n))
    assert res["rank_attempts"].tolist() == [int(want["attempts"].sum())]
    with pytest.raises(ValueError):
        parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY)                      # balanced, and nothing to balance by
    with pytest.raises(ValueError):
        parallel.sharded_sweep(eph, ship.start, pos, vel, ship.start + DAY, partition="random")
    empty = parallel.sharded_sweep(eph, ship.start, np.zeros((0, 3)), np.zeros((0, 3)), ship.start + DAY, partition="contiguous")
    assert empty["records"].shape == (0,) and empty["batch"].n == 0 and empty["balance"] == 1.0
