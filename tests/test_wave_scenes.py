"""CPU: the scenes of tests/wave_scenes.py on the restated tile walk and range test of wave_force (csrc/step_wave.hip), and on the two
oracles. Conditions, not measurements: each scene still takes the branch it was planted for (tests/test_gpu_wave_form.py compares the
device with the C oracle on these very scenes, so a scene that went quiet would check nothing)."""
import numpy as np
import pytest

import wave_scenes as ws
from oracle import orc, pyoracle

SIZES = sorted(set(ws.TILE_SIZES + ws.BPW_SIZES + (ws.N, 64, 65)))


def walk(n, i0):
    """wave_force's control flow, statement by statement (run / step / special of csrc/step_wave.hip), with the tiles as the values
    that travel through its registers and LDS buffers. Returns (events, summed): events = (tile, role) in the order the pair
    arithmetic of a tile is FINISHED, summed = the tiles in the order their contributions enter the ordered sum."""
    T = ws.TILE
    tiles, tfull, tdiag = (n + T - 1) // T, n // T, i0 // T
    events, summed = [], []

    def special(t):
        events.append((t, ws.SPECIAL))
        summed.append(t)

    def run(tb, te):
        if tb >= te:
            return
        buf, pre, src = [None, None], [None, None], [None, None]
        events.append((tb, ws.PROLOGUE))
        buf[0] = tb                                         # tile tb -> buffer 0
        pre[0] = min(tb + 1, te - 1)
        src[0], src[1] = min(tb + 2, te - 1), min(tb + 3, te - 1)
        steps = te - tb - 1
        done = [0]

        def step(ph, t):
            assert buf[ph] == t and pre[ph] == t + 1, (n, i0, t, buf, pre)
            done[0] += 1
            events.append((pre[ph], (ws.STEP, ph, done[0] == steps)))
            buf[ph ^ 1] = pre[ph]                           # contributions of tile t + 1 to the other buffer
            pre[ph ^ 1] = src[ph]                           # the hand-over
            summed.append(buf[ph])                          # the chain over buffer ph
            src[ph] = min(t + 4, te - 1)

        t = tb
        while t + 1 < te - 1:
            step(0, t)
            step(1, t + 1)
            t += 2
        if t < te - 1:
            step(0, t)
            summed.append(buf[1])
        else:
            summed.append(buf[0])
        assert done[0] == steps

    run(0, min(tdiag, tfull))
    special(tdiag)
    if tdiag < tfull:
        run(tdiag + 1, tfull)
        if tfull < tiles:
            special(tfull)
    return events, summed


@pytest.mark.parametrize("n", SIZES)
def test_schedule_is_the_kernels_walk(n):
    """every i0: each source tile finished once and summed once, in tile order; the roles are schedule()'s; a run [tb, te) has one
    prologue and te - tb - 1 steps whose phases alternate from 0 and whose last is the one flagged"""
    tiles = (n + ws.TILE - 1) // ws.TILE
    for i0 in range(n):
        events, summed = walk(n, i0)
        assert summed == list(range(tiles)), (n, i0, summed)
        assert [t for t, _ in events] == list(range(tiles)), (n, i0, events)
        role = ws.schedule(n, i0)
        assert dict(events) == role, (n, i0)
        lower, upper, specials = ws.runs(n, i0)
        assert [t for t, r in events if r == ws.SPECIAL] == specials and 1 <= len(specials) <= 2
        assert (i0 // ws.TILE in specials) and (n % ws.TILE == 0 or tiles - 1 in specials)
        for run in (lower, upper):
            if run is None or run[0] >= run[1]:
                continue
            tb, te = run
            mine = [role[t] for t in range(tb, te)]
            assert mine[0] == ws.PROLOGUE and len(mine) == te - tb
            assert [r[1] for r in mine[1:]] == [k & 1 for k in range(te - tb - 1)]
            assert [r[2] for r in mine[1:]] == [False] * (te - tb - 2) + [True] * (te - tb > 1)
            assert all(ws.run_of(i0, t) == ("lower" if run is lower else "upper") for t in range(tb + 1, te))


def test_the_sizes_reach_the_walks_they_are_there_for():
    """TILE_SIZES: whole numbers of tiles (no ragged special: the diagonal tile can be the last whole one) beside their ragged
    neighbours, and runs of five to seven tiles with the two-step loop turning more than once behind odd and even step counts.
    BPW_SIZES: no multiple of 8, one odd -- the last wave has clamped copies at BPW 2, 4 and 8; 705 has eleven whole tiles and a ragged one"""
    assert ws.TILE_SIZES == (128, 129, 191, 192, 193, 256, 320, 383, 384, 385, 448, 449, 511, 512)
    assert ws.BPW_SIZES == (65, 130, 131, 197, 330, 705)
    whole = [n for n in ws.TILE_SIZES if n % 64 == 0]
    assert whole == [128, 192, 256, 320, 384, 448, 512]
    for n in whole:
        lower, upper, specials = ws.runs(n, n - 1)         # tdiag == tfull - 1: nothing behind the wave's own tile
        assert specials == [n // 64 - 1] and upper == (n // 64, n // 64) and lower == (0, n // 64 - 1)

    def run_lengths(n):
        out = set()
        for i0 in list(range(0, n, 64)) + [n - 1]:
            lower, upper, _ = ws.runs(n, i0)
            out |= {te - tb for tb, te in (lower, upper or (0, 0)) if te > tb}
        return out
    assert [max(run_lengths(n)) for n in (384, 385, 448, 449, 511, 512)] == [5, 6, 6, 7, 7, 7]
    # a run of r tiles has r - 1 steps and turns the two-step loop (r - 1) // 2 times: 5, 6 and 7 tiles are 4, 5 and 6 steps
    assert {5, 6, 7} <= set().union(*(run_lengths(n) for n in ws.TILE_SIZES))
    assert all(n % 8 for n in ws.BPW_SIZES) and 131 % 2 == 1
    for bpw in (2, 4, 8):
        assert any(len(ws.wave_bodies(n, n - n % bpw, bpw)) < bpw for n in ws.BPW_SIZES)
        assert len(ws.wave_bodies(131, 131 - 131 % bpw, bpw)) == 131 % bpw
    assert 705 // 64 == 11 and 705 % 64 == 1


def test_range_test_restated():
    """the ends of the guarded ranges, and what each order tests beside n2"""
    for order, e in ((0, 300), (3, 300), (4, 133), (6, 133)):
        x = np.array([2.0 ** -e, np.nextafter(2.0 ** -e, 0.0), np.nextafter(2.0 ** e, 0.0), 2.0 ** e, 0.0, np.inf, np.nan, 5e-324])
        assert ws.n2_out_of_range(x, order).tolist() == [False, True, False, True, True, True, True, True], order
    mu = np.array([0.0, -0.0, 1e-70, 2.0 ** -200, np.nextafter(2.0 ** -200, 0.0), 1.0, np.nextafter(2.0 ** 200, 0.0), 2.0 ** 200])
    assert ws.mu_fails(mu, 4).tolist() == [True, True, True, False, True, False, False, True]
    assert ws.mu_fails(mu, 5).tolist() == [False, True, True, False, True, False, False, True]
    assert not ws.mu_fails(mu, 0).any() and not ws.mu_fails(mu, 6).any()
    pos = np.array([[0.0, 0.0, 0.0], [2.0 ** -500, 1.0, 1.0], [np.nextafter(2.0 ** -500, 0.0), 1.0, 1.0], [0.0, 1.0, 1.0]])
    one = np.ones(4)
    for order in (4, 6):                                    # a component below 2^-500 (its square below 2^-1000), or zero
        assert ws.fail_matrix(pos, one, order)[0].tolist() == [False, False, True, True]
    for order in (0, 5):
        assert not ws.fail_matrix(pos, one, order)[0].any()


def test_the_base_scene_never_leaves_the_range():
    pos, mu, _ = ws.base()
    assert len(set(mu.tolist())) == ws.N and mu.min() >= 1.0 and mu.max() <= 1e5 and (pos[10] == 0.0).all()
    for order in range(7):
        assert ws.failing_operands(pos, mu, order) == []
        for bpw in ws.BPWS:
            assert ws.fallback_steps(pos, mu, order, bpw) == set()


SCENES = {s.name: s for s in ws.scenes()}


def test_the_scenes_are_the_ones_asked_for():
    assert list(SCENES) == ["near(140,10)", "near(200,10)", "near(300,10)", "near(70,300)", "near(140,300)", "near(200,300)",
                            "far(140)", "far(200)", "far(300)", "massless(200)", "tiny_mass(200)", "coincident"]
    assert set(ws.STEPPED) <= set(SCENES)
    assert [s.planted for s in ws.near_scenes()] == [
        ((10, 2, 0, False, "upper"),), ((10, 3, 1, False, "upper"),), ((10, 4, 0, True, "upper"),),
        ((300, 1, 0, False, "lower"),), ((300, 2, 1, False, "lower"),), ((300, 3, 0, True, "lower"),)]
    assert SCENES["massless(200)"].mu[200] == 0.0 and SCENES["tiny_mass(200)"].mu[200] == 1e-70
    assert SCENES["massless(200)"].orders == (4,) and SCENES["tiny_mass(200)"].orders == (4, 5) and SCENES["coincident"].orders == (4, 6)
    # tile 3 is a tested step for the targets of tiles 0, 1, 4 and 5 (its own wave's special, tile 2's prologue)
    assert [ws.schedule(ws.N, 64 * d)[3] not in (ws.PROLOGUE, ws.SPECIAL) for d in range(6)] == [True, True, False, False, True, True]
    c = SCENES["coincident"]
    d = c.pos[262] - c.pos[5]
    assert d[0] == 0.0 and d[1] == 0.0 and d[2] == 1e7
    for s in (140, 200, 300):
        f = SCENES[f"far({s})"]
        d = f.pos[s] - f.pos[10]
        assert (d == (2.0 ** 151, 0.0, 0.0)).all() and (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == 2.0 ** 302


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("order", ws.ORDERS)
def test_scene_takes_the_fallback_it_was_planted_for(name, order):
    """in the orders a scene is planted for, at every BPW: fallback_steps holds the steps named, for the wave of the body named; in
    the other orders the scene stays on the fast sequences everywhere. A near scene has exactly two directed operands out of range
    (the planted pair, both ways) in every order; a far source is out of range for every wave"""
    sc = SCENES[name]
    failing = ws.failing_operands(sc.pos, sc.mu, order)
    if name.startswith("near"):
        s, body = (int(x) for x in name[5:-1].split(","))
        assert sorted(failing) == sorted([(body, s), (s, body)])
        d = sc.pos[s] - sc.pos[body]
        assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == 3 * 2.0 ** -302
    if name.startswith("far"):
        s = int(name[4:-1])
        assert sorted(failing) == sorted([(i, s) for i in range(ws.N) if i != s] + [(s, j) for j in range(ws.N) if j != s])
    for bpw in ws.BPWS:
        got = ws.fallback_steps(sc.pos, sc.mu, order, bpw)
        if order not in sc.orders:
            assert got == set() and failing == [], (name, order, bpw)
            continue
        assert got, (name, order, bpw)
        for body, tile, phase, last, run in sc.planted:
            i0 = ws.wave_of(body, bpw)
            assert (i0, tile, phase, last) in got and ws.run_of(i0, tile) == run, (name, order, bpw, body)
        if name.startswith("far"):                          # every wave whose walk steps through the far source's tile
            s = int(name[4:-1])
            stepped = {i0 for i0 in range(0, ws.N, bpw) if ws.schedule(ws.N, i0)[s // 64] not in (ws.PROLOGUE, ws.SPECIAL)}
            assert {i0 for i0, t, _, _ in got if t == s // 64} == stepped and len(stepped) >= 3 * 64 // bpw


@pytest.mark.parametrize("order", ws.ORDERS)
@pytest.mark.parametrize("bpw", ws.BPWS)
def test_the_scenes_cover_every_kind_of_step(order, bpw):
    """{phase 0, phase 1} x {last, not last} x {lower run, upper run}: all eight are fallen back in, in every order and at every BPW"""
    seen = set()
    for sc in ws.scenes():
        seen |= {(phase, last, ws.run_of(i0, tile)) for i0, tile, phase, last in ws.fallback_steps(sc.pos, sc.mu, order, bpw)}
    assert seen == {(p, last, run) for p in (0, 1) for last in (False, True) for run in ("lower", "upper")}


@pytest.fixture(scope="module")
def python_scene():
    """a scene as pyoracle takes it"""
    def convert(sc):
        return [pyoracle.Vec(*map(float, r)) for r in sc.pos], [float(m) for m in sc.mu]
    return convert


@pytest.mark.parametrize("name", list(SCENES))
def test_c_oracle_equals_the_python_restatement_on_the_scene(name, python_scene):
    """orders 0, 4, 5, 6: the two independent restatements agree bit for bit, and every acceleration is finite"""
    sc = SCENES[name]
    y, mu = python_scene(sc)
    try:
        for order in ws.ORDERS:
            orc.set_pair_variant(order)
            pyoracle.set_pair_variant(order)
            c = orc.gravity(sc.pos, sc.mu)
            p = np.array([list(v) for v in pyoracle.gravity(y, mu, 0.0)])
            assert np.isfinite(c).all(), (name, order)
            ws.assert_same(c, p, f"{name}, order {order}: C oracle against pyoracle")
    finally:
        orc.set_pair_variant(0)
        pyoracle.set_pair_variant(0)


def test_the_comparison_names_what_differs():
    sc = SCENES["far(140)"]
    a = orc.gravity(sc.pos, sc.mu)
    ws.assert_same(a, a.copy(), "self")
    b = a.copy()
    b[17, 1] = np.nextafter(b[17, 1], np.inf)
    with pytest.raises(AssertionError, match=r"flipped: body 17 \(1 of 330 bodies differ\)"):
        ws.assert_same(b, a, "flipped")


@pytest.mark.parametrize("name", ws.STEPPED)
@pytest.mark.parametrize("order", ws.ORDERS)
def test_the_stepped_scenes_stay_finite_and_out_of_range(name, order):
    """the 12 + 3 steps the GPU file takes on them: the oracle's state and accelerations stay finite, and the positions it ends on
    still send waves through the fallback (the near pair is flung apart by its first evaluation: out of range at the far end)"""
    sc = SCENES[name]
    orc.set_pair_variant(order)
    try:
        o = orc.NBody(sc.pos, ws.velocities(), sc.mu, 0.0, ws.H, "QuinlanTremaine12")
        assert o.advance(12 + 3) == 0
        pos, vel, _, steps = o.state()
        assert steps == 15 and np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(o.acc()).all()
        for bpw in ws.BPWS:
            assert ws.fallback_steps(pos, sc.mu, order, bpw), (name, order, bpw)
    finally:
        orc.set_pair_variant(0)
