"""-m gpu: the 14 / 14 / 14 / 6 deal of the 16-body workgroup kernel (csrc/step_wg.hip) and the ends of the guarded range of the
staged term (csrc/pair_term.h: pair_finish_staged).

In every three-tile phase the rank-2 pair wave of SIMDs 1-3 carries four bodies against the phase's third tile and wave 8 (the tail
wave of k_lm_step_wg, an otherwise idle wave of k_accel_wg) carries local bodies 5, 10 and 15 against that tile as one three-body
block. The kernel is forced (EPH_FORCE=wg EPH_WG_BODIES=16, read once per process: hence the child processes); the evaluation
order comes from EPH_PAIR_VARIANT in the child's environment. Everything is bit for bit against the CPU oracle.

Third tiles: tile t is the third tile of a phase when t = 4, 7, 10, ... (phases: {0}, {1}, {2, 3, 4}, {5, 6, 7}, ...)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_step_phases import FORCED, PRELUDE, _free_port, _shard_worker

pytestmark = pytest.mark.gpu

# the wave's range test as the kernel makes it (csrc/pair_term.h: kRangeBase / kRangeSpan, range_key; kLowSq, low_key)
RANGE = r'''
import os
K = int(os.environ.get("EPH_PAIR_VARIANT", "0"))
orc.set_pair_variant(K)
assert ea.pair_variant() == K
BASE, SPAN = (0x37A00000, 0x10A00000) if K >= 4 else (0x2D300000, 0x25800000)
LOWSQ = 0x01700000
hi = lambda x: int(np.float64(x).view(np.uint64)) >> 32
def n2_of(pos, i, j):                                  # d = p_other - p_self, squares summed left to right
    d = pos[j] - pos[i]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], d
out_of_range = lambda n2: ((hi(n2) - BASE) & 0xffffffff) >= SPAN
def all_n2(pos):
    d = pos[None, :, :] - pos[:, None, :]
    n2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return n2[~np.eye(len(pos), dtype=bool)]
'''


def run_forced(script, *args, variant=0):
    env = dict(os.environ, **FORCED)
    env["EPH_PAIR_VARIANT"] = str(variant)
    r = subprocess.run([sys.executable, "-c", PRELUDE + RANGE + script, str(ROOT), *map(str, args)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_third_tiles(gpu):
    """n = 300: tile 4 is the first third tile and ragged; the workgroup of bodies 288-299 has its local body 15 absent (and 12-14:
    clamped copies of body 299) and its own tile IS that third tile -- the three-body block takes the IEEE form. 320 / 321: tile 4
    whole. 449, 512, 513: tile 7 ragged / whole, 513 with a one-tile last phase behind it. 705: last workgroup partly empty."""
    run_forced(r'''
rng = np.random.default_rng(21)
for n in (300, 320, 321, 449, 512, 513, 705):
    pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
    assert same(ea.accel_eval(pos, mu), orc.gravity(pos, mu)), ("accel", n)
print("ok")
''')


def test_fused_steps(gpu):
    """k_lm_step_wg<12, 16>: the tail wave carries the block beside its 24 history values; <13, 16> (Stormer13): beside 26"""
    run_forced(r'''
for n, method in ((300, "QuinlanTremaine12"), (330, "QuinlanTremaine12"), (513, "QuinlanTremaine12"), (330, "Stormer13")):
    pos, vel, mu = plummer(n)
    g = ea.NBodyIntegration(pos, vel, mu, 0.0, 1.0 / 1024.0, method)
    o = orc.NBody(pos, vel, mu, 0.0, 1.0 / 1024.0, method, native=True)
    steps = (13 if method == "Stormer13" else 12) + 7
    g.advance(steps)
    assert o.advance(steps) == 0
    assert same(g.state()[0], o.state()[0]) and same(g.state()[1], o.state()[1]), ("steps", n, method)
print("ok")
''')


@pytest.mark.parametrize("variant", [0, 4, 5])
def test_slow_path_on_the_three_body_block(gpu, variant):
    """n = 330 (tiles 0-5; tile 4 = sources 256-319 is the third tile of phase {2, 3, 4}); the block of workgroup 0 is bodies 5, 10,
    15. Body 10 sits at the origin. (a) source 260 at 2^151 along x from body 10, equal to it in y and z: n2 = 2^302, above the
    guarded range of every order, and two zero components. (Such a source is as far from every other body, so the four-body waves
    meeting tile 4 take the IEEE form with it.) (b) source 261 at 2^-151 from body 10 along every axis: n2 = 3 * 2^-302, below
    every guarded range, for body 10 ONLY -- the block takes the IEEE form, the four-body waves on the same tile do not.
    (c) source 262 coincident with body 5 in x and y: n2 in range, two component differences +0; orders 4 and 6 divide the
    components, so for order 4 this is the low_key exit. The planted operands are checked against the kernel's range test
    here, so that the branch is known to be taken."""
    run_forced(r'''
rng = np.random.default_rng(22)
n = 330
base, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
base[10] = 0.0
far = base.copy()
far[260] = (2.0 ** 151, 0.0, 0.0)
n2, d = n2_of(far, 10, 260)
assert n2 == 2.0 ** 302 and out_of_range(n2) and d[1] == 0.0 and d[2] == 0.0, ("far: planted n2 in range", K, n2)
assert same(ea.accel_eval(far, mu), orc.gravity(far, mu)), ("far source", K)
near = base.copy()
near[261] = 2.0 ** -151
n2, d = n2_of(near, 10, 261)
assert n2 == 3 * 2.0 ** -302 and out_of_range(n2), ("near: planted n2 in range", K, n2)
others = np.array([n2_of(near, i, j)[0] for i in range(16) for j in range(256, 320) if (i, j) != (10, 261)])
assert not any(out_of_range(v) for v in others), "body 10 against source 261 is meant to be the only operand out of range"
assert same(ea.accel_eval(near, mu), orc.gravity(near, mu)), ("near source", K)
zero = base.copy()
zero[262] = (base[5][0], base[5][1], base[5][2] + 1e7)
n2, d = n2_of(zero, 5, 262)
assert d[0] == 0.0 and d[1] == 0.0 and not out_of_range(n2), ("coincident", K, n2, d)
if K in (4, 6):                                         # the squares of the components: the smallest high word below 2^-1000's
    assert min(hi(d[0] * d[0]), hi(d[1] * d[1]), hi(d[2] * d[2])) < LOWSQ
assert same(ea.accel_eval(zero, mu), orc.gravity(zero, mu)), ("coincident source", K)
print("ok")
''', variant=variant)


@pytest.mark.parametrize("variant", [0, 5])
def test_range_ends_of_the_staged_term(gpu, variant):
    """Written for scripts/experiments/pair_expadd.patch (the two power-of-two scalings of pair_finish_staged as integer adds on
    the exponent field: exact only while operands and results are normal, which the guarded range [2^-300, 2^300) of n2 is there
    to ensure; orders 4-6: [2^-133, 2^133)); it holds the shipped multiplications to the same ends of the range. n = 130 on
    a jittered 6 x 6 x 4 lattice, scaled so that the SMALLEST n2 lies just above 2^-299, then so that the LARGEST lies just
    below 2^299; mu in [1, 1e5): 1 / p is within 2^+-450 and mu / p, d * (mu / p) stay normal.

    (The wording "every n2 in [2^-299, 2^-297]" cannot be met: no more than about a dozen points of space have all their mutual
    squared distances within a factor of four. What is asserted instead, before the comparison: every n2 inside the guarded range
    of order 0, so every wave but those meeting its own tile stays on the staged sequence, and the extreme n2 -- the operand
    nearest the range end, some hundreds of pairs -- inside the band asked for.) Order 5's own guarded range ends at 2^+-133:
    it is run at ITS ends in the same way (bands [2^-132, 2^-130) and (2^130, 2^132]), and at order 0's ends as well, where its
    waves all take the IEEE form."""
    run_forced(r'''
rng = np.random.default_rng(23)
n = 130
idx = np.arange(n)
pos0 = np.stack([idx % 6, (idx // 6) % 6, idx // 36], axis=1) + rng.uniform(-0.2, 0.2, size=(n, 3))
mu = rng.uniform(1.0, 1e5, n)
n2 = all_n2(pos0)
for end in sorted({300, 133 if K >= 4 else 300}):
    # the smallest n2 just above 2^-(end - 1), then the largest just below 2^(end - 1)
    for f, low in ((np.sqrt(1.01 * 2.0 ** -(end - 1) / n2.min()), True), (np.sqrt(0.99 * 2.0 ** (end - 1) / n2.max()), False)):
        pos = pos0 * f
        v = all_n2(pos)
        assert v.min() >= 2.0 ** -end and v.max() < 2.0 ** end, ("outside the guarded range", K, end, low)
        if low:
            band = (v >= 2.0 ** -(end - 1)) & (v < 2.0 ** -(end - 3))
            assert 2.0 ** -(end - 1) <= v.min() < 2.0 ** -(end - 3) and band.sum() >= 100, (K, end, np.log2(v.min()), band.sum())
        else:
            band = (v > 2.0 ** (end - 3)) & (v <= 2.0 ** (end - 1))
            assert 2.0 ** (end - 3) < v.max() <= 2.0 ** (end - 1) and band.sum() >= 100, (K, end, np.log2(v.max()), band.sum())
        if end == (133 if K >= 4 else 300):
            assert not any(out_of_range(x) for x in (v.min(), v.max())), ("the order's own range test", K, end)
        a = ea.accel_eval(pos, mu)
        assert np.all(np.isfinite(a)) and np.all(np.abs(a[a != 0]) >= 2.0 ** -1022), ("a product left the normal range", K, end, low)
        assert same(a, orc.gravity(pos, mu)), ("range end", K, end, "low" if low else "high")
print("ok")
''', variant=variant)


def test_target_partition_cut_inside_a_workgroup(gpu, monkeypatch):
    """eph_nbody_shard, two ranks through the host-staged exchange at n = 712 (768 padded: 384 targets per rank). The library cuts
    at multiples of 64 / world, so a range can end inside a workgroup only at hi = n: the second rank's last workgroup (bodies
    704-711 of 704-719) has local bodies 0-7, the cut falling between the block's bodies 5 and 10 -- the block computes one live body
    and two clamped copies, the rank-2 waves live and clamped rows alike. 12 + 7 steps, bit-identical to the single handle."""
    import torch.multiprocessing as mp
    for k, v in FORCED.items():
        monkeypatch.setenv(k, v)
    n, world, steps = 712, 2, 7
    assert 5 < n % 16 <= 10
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_shard_worker, args=(world, _free_port(), n, steps, out), nprocs=world, join=True)
    (p0, v0, t0, sc0), a0 = out["single"]
    for r in range(world):
        (p, v, t, sc), a, (lo, hi, gathers) = out[r]
        assert (lo, hi) == (r * 384, min(n, (r + 1) * 384)) and gathers > 0
        assert t == t0 and sc == sc0
        assert np.array_equal(p, p0) and np.array_equal(v, v0) and np.array_equal(a, a0), r
