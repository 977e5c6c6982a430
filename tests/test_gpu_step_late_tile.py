"""-m gpu: the late third tile of the 16-body workgroup kernel (csrc/step_wg.hip, the comment above phase_start).

Phases 0 and 1 are the single tiles 0 and 1; phase P >= 2 holds tiles 3 P - 4 .. 3 P - 2, called a, b, c. Every producer of a c
(the rank-2 pair waves, the three-body block of wave 8, the third interaction of the one-body wave) computes it in its phase's
interval, keeps it in registers across the barrier and writes it inside the next interval; the chain wave sums {c(P - 1), a(P),
b(P)} behind barrier P, and a c that is the last tile alone behind one more barrier. The c tiles are t = 4, 7, 10, ...
Evaluation orders 0, 4 and 5 have this schedule (kWgLateThird); the others write c before its phase's barrier as before.

The kernel is forced (EPH_FORCE=wg EPH_WG_BODIES=16, read once per process: hence the child processes); everything is bit for bit
against the CPU oracle."""
import numpy as np
import pytest

from test_gpu_step_phases import FORCED, _free_port, _shard_worker
from test_gpu_step_units import run_forced

pytestmark = pytest.mark.gpu


def test_accelerations_by_number_of_late_tiles(gpu):
    """k_accel_wg<16> by tile count. No c at all: n = 64, 128, 192, 256 (1-4 tiles). One c that is also the last tile, summed
    alone behind the additional barrier: 320 (whole) and 300 (ragged). A c followed by a short last phase, where the held tile is
    written with no block around the writes: 384 (one tile behind it) and 448 (two). Two c's, the first written inside the block
    of the second: 449 (8 tiles, tile 7 holds ONE source), 512 (tile 7 whole and last), 513 (a one-tile phase behind tile 7).
    Three c's: 705 (12 tiles, the last workgroup partly empty)."""
    run_forced(r'''
rng = np.random.default_rng(31)
tiles = lambda n: (n + 63) // 64
late = lambda n: len([t for t in range(4, tiles(n), 3)])
expect = {64: 0, 128: 0, 192: 0, 256: 0, 300: 1, 320: 1, 384: 1, 448: 1, 449: 2, 512: 2, 513: 2, 705: 3}
for n, cs in expect.items():
    assert late(n) == cs, (n, late(n))
    pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
    assert same(ea.accel_eval(pos, mu), orc.gravity(pos, mu)), ("accel", n)
print("ok")
''')


def test_own_tile_in_every_position_of_a_phase(gpu):
    """n = 513 (tiles 0-8): the workgroup of bodies i0 .. i0 + 15 has its own tile tdiag = i0 // 64, whose waves take the IEEE form
    and whose sums the chain wave takes masked. tdiag = 2 and 5 are an a, 3 and 6 a b, 4 and 7 a c (the IEEE results held over the
    barrier), 8 the one-tile last phase. Every workgroup is compared on its own."""
    run_forced(r'''
rng = np.random.default_rng(32)
n = 513
pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
got, want = ea.accel_eval(pos, mu), orc.gravity(pos, mu)
role = lambda t: "single" if t < 2 else "abc"[(t - 2) % 3]
seen = set()
for i0 in range(0, n, 16):
    seen.add((i0 // 64, role(i0 // 64)))
    assert same(got[i0:i0 + 16], want[i0:i0 + 16]), ("workgroup", i0, "own tile", i0 // 64, role(i0 // 64))
assert {(2, "a"), (3, "b"), (4, "c"), (5, "a"), (6, "b"), (7, "c"), (8, "a")} <= seen
print("ok")
''')


def test_fused_steps(gpu):
    """k_lm_step_wg<12, 16> and <13, 16> (the tail wave holds nine doubles over the barrier beside its 24 / 26 history values):
    12 + 7 steps at n = 330 (one c, a one-tile phase behind it) and 513 (two c's), 13 + 7 of Stormer13 at 330; k_accel_wg<16> at
    the same sizes on the final positions."""
    run_forced(r'''
for n, method in ((330, "QuinlanTremaine12"), (513, "QuinlanTremaine12"), (330, "Stormer13")):
    pos, vel, mu = plummer(n)
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, 1.0 / 1024.0, method)
    o = orc.NBody(pos, vel, mu, 0.0, 1.0 / 1024.0, method, native=True)
    steps = (13 if method == "Stormer13" else 12) + 7
    g.advance(steps)
    assert o.advance(steps) == 0
    assert same(g.state()[0], o.state()[0]) and same(g.state()[1], o.state()[1]), ("steps", n, method)
    p = np.ascontiguousarray(o.state()[0])
    assert same(ea.accel_eval(p, mu), orc.gravity(p, mu)), ("accel", n, method)
print("ok")
''')


@pytest.mark.parametrize("variant", [0, 4, 5])
def test_slow_path_on_a_late_tile(gpu, variant):
    """One planted operand outside the guarded ranges in a c tile, as test_slow_path_on_the_three_body_block plants it: body 10
    (of wave 8's block in workgroup 0) at the origin and ONE source 2^-151 away from it along every axis, n2 = 3 * 2^-302, below
    the guarded range of every order for that pair and no other of the tile. n = 513, c tiles 4 (sources 256-319) and 7 (448-511):
    planted in tile 4 the block's IEEE results are held and then written by the staged block of tile 7; planted in tile 7 the
    block of tile 7 writes the held tile 4 on its IEEE side and its own results go out with no block around them. Then the whole
    tile: a source 2^151 away along x, out of range for every body, so every producer of that c takes the IEEE form."""
    run_forced(r'''
rng = np.random.default_rng(33)
n = 513
base, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
base[10] = 0.0
for src in (261, 450):
    lo = src // 64 * 64
    assert (lo // 64 - 4) % 3 == 0, "a c tile"
    near = base.copy()
    near[src] = 2.0 ** -151
    n2, d = n2_of(near, 10, src)
    assert n2 == 3 * 2.0 ** -302 and out_of_range(n2), ("near: planted n2 in range", K, n2)
    others = np.array([n2_of(near, i, j)[0] for i in range(16) for j in range(lo, lo + 64) if (i, j) != (10, src)])
    assert not any(out_of_range(v) for v in others), "body 10 against the planted source is meant to be the only operand out of range"
    assert same(ea.accel_eval(near, mu), orc.gravity(near, mu)), ("near source", K, src)
    far = base.copy()
    far[src] = (2.0 ** 151, 0.0, 0.0)
    n2, d = n2_of(far, 10, src)
    assert n2 == 2.0 ** 302 and out_of_range(n2), ("far: planted n2 in range", K, n2)
    assert same(ea.accel_eval(far, mu), orc.gravity(far, mu)), ("far source", K, src)
print("ok")
''', variant=variant)


def test_target_partition_cut_inside_a_workgroup(gpu, monkeypatch):
    """eph_nbody_shard, two ranks through the host-staged exchange at n = 712 (12 tiles: c tiles 4, 7, 10; 384 targets per rank).
    The library cuts at multiples of 64 / world, so a range ends inside a workgroup only at hi = n: the second rank's last
    workgroup (bodies 704-711 of 704-719) holds clamped copies over the barrier like live rows. 12 + 7 steps, bit-identical to the
    single handle."""
    import torch.multiprocessing as mp
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    n, world, steps = 712, 2, 7
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), n, steps, out), nprocs=world, join=True)
    (p0, v0, t0, sc0), a0 = out["single"]
    for r in range(world):
        (p, v, t, sc), a, (lo, hi, gathers) = out[r]
        assert (lo, hi) == (r * 384, min(n, (r + 1) * 384)) and gathers > 0
        assert t == t0 and sc == sc0
        assert np.array_equal(p, p0) and np.array_equal(v, v0) and np.array_equal(a, a0), r
