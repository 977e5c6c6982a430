"""Scenes for the small workgroup forms of csrc/step_wg.hip off their fast path, shared by tests/test_wg_small_scenes.py (CPU: every
scene reaches the branch it names, on the restated schedule) and tests/test_gpu_wg_small_forms.py (the kernels against the C oracle,
bit pattern against bit pattern). A plain module: no fixtures, no GPU import. The range test of a pair wave is NOT restated here: it
is fail_matrix of tests/wave_scenes.py (range_key / mu_key / low_key of csrc/pair_term.h), pinned by tests/test_wave_scenes.py.

    form   kernel side                                                  bodies per workgroup   unit of one range test (one ballot)
    wg4    wg_force_split: wg_pair_wave<1> -> wg_pair_tile<1>           4                      one body, one tile t, every t < tiles
    wg8    wg_pair_wave_big<1> (twelve waves)                           8                      one body, big tile K
    duo    wg_pair_wave_big<2> (six waves; k_lm_step_wg<L, 8, true>)    8                      bodies i0 + 2 w and i0 + 2 w + 1, big tile K

The schedule, restated from the code. A workgroup is the bodies i0 .. i0 + WB - 1 with i0 = lo + WB * block (lo = 0: one device) and
tdiag = i0 // 64; bodies past n - 1 are copies of body n - 1 (wg_load_own, and the loop written out in wg_pair_wave_big). Lane l of
tile t holds source min(64 t + l, n - 1) (load_src): the padding lanes of a ragged last tile take part in the ballot as copies of
source n - 1. Big tiles (big_start, big_count, `produce`): {0} and {1} are single tiles; big tile K >= 2 starts at tile 2 K - 2 and
is the pair {2 K - 2, 2 K - 1} through wg_pair_tile2 when 2 K - 1 < tiles, else the single last tile {2 K - 2} through wg_pair_tile
like {0} and {1}. A unit that contains tdiag goes to the IEEE form whatever its operands (`ieee`): it is not a TESTED unit.

What is planted, and for what (n = 330: six tiles, big tiles {0} {1} {2,3} {4,5}, tile 5 ragged with 10 sources):

  near(s, body)        `body` at the origin, source s 2^-151 from it on every axis: n2 = 3 * 2^-302, below every order's guarded range,
                       for that pair alone -- exactly two tested units fail, the two directed halves, beside fast units in the same
                       launch. body 10 with s = 140, 300 (first tile of a pair), 200 (second), 325 (ragged second); bodies 11 and 301
                       with s = 200: the operand belongs to the SECOND body of a duo wave only; body 300 with s = 70 and 20: the
                       single tiles 1 and 0 of the big schedule for a body whose own tile is neither; near(329, 10): the source is
                       the clamp body, and the last workgroup's clamped copies of it fail as well.
  far(s)               source s at (2^151, 0, 0), body 10 at the origin: the unit that holds s's tile fails for EVERY workgroup.
                       s = 200 and s = 329 (the padding lanes of tile 5 carry the out-of-range copy).
  far(s, 2^400)        the same 2^400 away: n2 = 2^800 and p = n2 sqrt(n2) OVERFLOWS. The IEEE term is mu / inf = +0 for every order,
                       so every result stays finite, while the wrapper-free sequences return NaN (fma(-inf, 0, 1)): an operand for
                       which taking the fast branch by mistake CHANGES THE BITS (2^151, 3 * 2^-302, a massless or tiny source and a
                       zero component are all outside the GUARDED ranges but inside the range where the sequences are still exact:
                       profiles/wg_small_forms.md). s = 201: second tile of a pair, and as a body the SECOND of its duo wave;
                       s = 140: first tile; s = 271 at n = 280: the last single tile.
  faint_tile(3)        the same for mu_key: only tile 3 (second of a pair) has mass, and a subnormal one. Orders 4 and 5.
  thin_tile(3)         the same for low_key: only tile 3 has mass, and every dx against it is subnormal. Orders 4 and 6.
  massless(s)          mu[s] = 0: order 4 only.   tiny_mass(s): mu[s] = 1e-70: orders 4 and 5. s = 140 (first), 200 (second), 325 (ragged).
  coincident(s, body)  source s equal to `body` in x and y: orders 4 and 6 through low_key. (262, 5): first; (200, 5): second.

n = 280: five tiles, the last big tile is the single ragged tile 4 through wg_pair_tile. n = 600 and n = 1100: the sizes dispatch.cpp
itself gives to wg4 and to wg8 / duo."""
from collections import namedtuple

import numpy as np

import wave_scenes as ws
from wave_scenes import Scene, assert_same, assert_same_run, base, fail_matrix, hi_word, mu_fails, range_consts  # noqa: F401

TILE = 64
N = ws.N
ORDERS = ws.ORDERS
FORMS = {"wg4": 4, "wg8": 8, "duo": 8}                        # form: bodies per workgroup
FORCED = {"wg4": 4, "wg8": 8, "duo": 9}                       # form: EPH_WG_BODIES
METHODS = ws.METHODS
QUIET_H = 2.0 ** -400                                         # the quiet step: the planted operands survive the start-up
SINGLE, FIRST, SECOND = "single", "first", "second"
FAR_OVERFLOW = 400                                            # a source 2^400 away: n2 = 2^800, and p = n2 sqrt(n2) overflows


# ---- the schedule, restated
def tile_count(n):
    return (n + TILE - 1) // TILE


def big_tiles(tiles):
    """the big tiles of wg_pair_wave_big as tuples of tiles: K < big_count(tiles), from big_start(K); a pair when its second tile exists"""
    count = tiles if tiles <= 2 else 2 + (tiles - 2 + 1) // 2
    out = []
    for K in range(count):
        t = K if K < 2 else 2 * K - 2
        out.append((t, t + 1) if K >= 2 and t + 1 < tiles else (t,))
    return out


def position(n, t, form):
    """(where tile t stands in its unit: SINGLE | FIRST | SECOND, is it ragged)"""
    ragged = TILE * (t + 1) > n
    if form == "wg4":
        return SINGLE, ragged
    group = next(g for g in big_tiles(tile_count(n)) if t in g)
    return (SINGLE if len(group) == 1 else (FIRST, SECOND)[group.index(t)]), ragged


def lane_sources(n, t):
    """the 64 sources the lanes of tile t hold"""
    return np.minimum(TILE * t + np.arange(TILE), n - 1)


Unit = namedtuple("Unit", "i0 slot bodies tiles")             # slot: the local body (wg4, wg8) or the pair wave (duo)


def units(n, form):
    """every unit of a launch over all n targets -> (unit, tested): tested = it does not contain the workgroup's own tile"""
    wb, tiles = FORMS[form], tile_count(n)
    groups = [(t,) for t in range(tiles)] if form == "wg4" else big_tiles(tiles)
    for i0 in range(0, n, wb):
        if form == "duo":
            slots = [(w, (min(i0 + 2 * w, n - 1), min(i0 + 2 * w + 1, n - 1))) for w in range(4)]
        else:
            slots = [(b, (min(i0 + b, n - 1),)) for b in range(wb)]
        for slot, bodies in slots:
            for g in groups:
                yield Unit(i0, slot, bodies, g), i0 // TILE not in g


def operand_fails(pos, mu, order):
    """fail_matrix with the self operand failing as well (n2 = 0 is below every range): a clamped copy can meet itself"""
    bad = fail_matrix(pos, mu, order)
    bad[np.diag_indices(len(bad))] = True
    return bad


def failing_units_of(bad, form):
    """failing_units from the matrix of failing operands"""
    n = len(bad)
    by_tile = np.stack([bad[:, lane_sources(n, t)].any(axis=1) for t in range(tile_count(n))], axis=1)   # [body, tile]
    out = {}
    for u, tested in units(n, form):
        if tested:
            carriers = tuple(t for t in u.tiles if any(by_tile[b, t] for b in u.bodies))
            if carriers:
                out[u] = carriers
    return out


def failing_units(scene, order, form, pos=None):
    """{tested unit whose one ballot fails: the tiles of it that carry a failing operand}; pos: other positions than the scene's"""
    return failing_units_of(operand_fails(scene.pos if pos is None else pos, scene.mu, order), form)


def in_range_operands(bad, unit):
    """how many of the unit's operands (bodies x lanes of its tiles) pass the range test"""
    cols = np.concatenate([lane_sources(len(bad), t) for t in unit.tiles])
    return int((~bad[list(unit.bodies)][:, cols]).sum())


def unit_of(n, form, body, tile):
    """the unit in which the workgroup that OWNS `body` meets `tile`"""
    wb = FORMS[form]
    i0 = body - body % wb
    slot = (body - i0) // 2 if form == "duo" else body - i0
    return next(u for u, _ in units(n, form) if u.i0 == i0 and u.slot == slot and tile in u.tiles)


# ---- scenes
def system(n):
    """n bodies ~1e7 apart, distinct mu in [1, 1e5], body 10 at the origin, and the row body 10 was drawn with; n = 330: ws.base()"""
    if n == N:
        return base()
    rng = np.random.default_rng(n)
    pos, mu = rng.normal(size=(n, 3)) * 1e7, rng.uniform(1.0, 1e5, n)
    drawn = pos[10].copy()
    pos[10] = 0.0
    return pos, mu, drawn


def _scene(name, n, pos, mu, orders, planted, where):
    """planted: the directed operands (body, source) whose units must fail; where: (SINGLE | FIRST | SECOND, ragged) of the source's
    tile on the big schedule"""
    sc = Scene(name if n == N else f"{name}@{n}", pos, mu, orders, planted)
    sc.n, sc.where, sc.still = n, where, False               # still: the velocities of a quiet step underflow to zero
    return sc


def near(s, body=10, n=N):
    pos, mu, drawn = system(n)
    if body != 10:
        pos[10] = drawn
        pos[body] = 0.0
    pos[s] = 2.0 ** -151
    return _scene(f"near({s},{body})", n, pos, mu, ORDERS, [(body, s), (s, body)], position(n, s // TILE, "wg8"))


def far(s, n=N, e=151):
    pos, mu, _ = system(n)
    pos[s] = (2.0 ** e, pos[10][1], pos[10][2])
    return _scene(f"far({s})" if e == 151 else f"far({s},2^{e})", n, pos, mu, ORDERS, [(10, s)], position(n, s // TILE, "wg8"))


def _a_body_elsewhere(n, s):
    """a body whose workgroup's own tile is not in the big tile of source s: its unit with that tile is tested"""
    group = next(g for g in big_tiles(tile_count(n)) if s // TILE in g)
    return 10 if 0 not in group else 300


def massless(s, n=N):
    pos, mu, _ = system(n)
    mu[s] = 0.0
    return _scene(f"massless({s})", n, pos, mu, (4,), [(_a_body_elsewhere(n, s), s)], position(n, s // TILE, "wg8"))


def tiny_mass(s, n=N):
    pos, mu, _ = system(n)
    mu[s] = 1e-70
    return _scene(f"tiny_mass({s})", n, pos, mu, (4, 5), [(_a_body_elsewhere(n, s), s)], position(n, s // TILE, "wg8"))


def coincident(s, body, n=N):
    pos, mu, _ = system(n)
    pos[s] = (pos[body][0], pos[body][1], pos[body][2] + 1e7)
    return _scene(f"coincident({s},{body})", n, pos, mu, (4, 6), [(body, s), (s, body)], position(n, s // TILE, "wg8"))


SHRINK = 2.0 ** -43                                           # positions ~2^-20: n2 ~ 2^-40, inside every guarded range; p ~ 2^-60


def _tile_bodies(n, t):
    return np.arange(TILE * t, min(TILE * t + TILE, n))


def faint_tile(t, n=N):
    """the system shrunk to 2^-20, every mass +0 but those of tile t, which are SUBNORMAL (about 2^-1040). Order 5 lets the +0
    masses pass, so only the units holding tile t fail (order 4: every unit). The accelerations are the sums of tile t's terms
    alone (about 2^-1000, normal), and for a subnormal numerator the residual of the division step underflows: on these operands the
    wrapper-free quotient is NOT the IEEE quotient (tests/test_wg_small_scenes.py counts them in exact arithmetic), so a unit that
    skipped mu_key shows in the last bit of the result. The velocities of a quiet step underflow: acc() carries the bits"""
    pos, _, _ = system(n)
    mu = np.zeros(n)
    mu[_tile_bodies(n, t)] = np.random.default_rng([n, t]).uniform(1.0, 2.0, len(_tile_bodies(n, t))) * 2.0 ** -1040
    sc = _scene(f"faint_tile({t})", n, pos * SHRINK, mu, (4, 5), [(_a_body_elsewhere(n, TILE * t), TILE * t + 5)],
                position(n, t, "wg8"))
    sc.still = True
    return sc


def thin_tile(t, n=N):
    """the shrunk system again, every mass +0 but those of tile t (ordinary ones), and every x a SUBNORMAL number -- but in the
    tile that shares a big tile with t, where x is about 2^-400. Against tile t every dx is subnormal and its square 0: low_key
    fails (orders 4 and 6), while the operands of the partner tile pass. The x component of an acceleration is the sum of tile
    t's terms alone, and for a subnormal numerator dx the wrapper-free quotient is not the IEEE quotient: a unit that took `low`
    from its first tile only shows in the last bit of x. (Order 4 fails everywhere: it tests the +0 masses.)"""
    pos, mu, _ = system(n)
    rng = np.random.default_rng([n, t, 1])
    pos = pos * SHRINK
    pos[:, 0] = rng.integers(-2 ** 30, 2 ** 30, n) * 2.0 ** -1074
    for partner in (u for g in big_tiles(tile_count(n)) if t in g for u in g if u != t):
        rows = _tile_bodies(n, partner)
        pos[rows, 0] = rng.uniform(1.0, 2.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)) * 2.0 ** -400
    mass = np.zeros(n)
    mass[_tile_bodies(n, t)] = mu[_tile_bodies(n, t)]
    return _scene(f"thin_tile({t})", n, pos, mass, (4, 6), [(_a_body_elsewhere(n, TILE * t), TILE * t + 5)], position(n, t, "wg8"))


def scenes_330():
    return ([near(s) for s in (140, 200, 300, 325)] + [near(200, 11), near(200, 301), near(70, 300), near(20, 300), near(329, 10)]
            + [far(200), far(329), far(201, e=FAR_OVERFLOW), far(140, e=FAR_OVERFLOW)] + [massless(s) for s in (140, 200, 325)] + [tiny_mass(s) for s in (140, 200, 325)]
            + [coincident(262, 5), coincident(200, 5), faint_tile(3), thin_tile(3)])


def scenes_280():
    return [near(270, 10, 280), far(279, 280), far(271, 280, FAR_OVERFLOW)]


def scenes_natural(n):
    """n = 600 (ten tiles, tile 9 ragged) and n = 1100 (eighteen, tile 17 ragged): a near source in the second tile of a pair, one in
    the ragged last tile, the clamp body far away, a tiny mass in an odd tile"""
    return [near(200, 10, n), near(n - 5, 10, n), far(n - 1, n), tiny_mass(350, n), far(201, n, FAR_OVERFLOW)]


NATURAL_SIZES = {600: "wg4", 1100: "duo"}                     # n: the form dispatch.cpp gives its fused step
NATURAL_ORDERS = (0, 4)


def scenes():
    return scenes_330() + scenes_280() + scenes_natural(600) + scenes_natural(1100)


def scene(name):
    return {s.name: s for s in scenes()}[name]


STORMER = "near(200,11)"                                      # the scene that is also stepped with Stormer13


def zero_velocities(n):
    return np.zeros((n, 3))


# ---- the range ends of the staged term at M = 2 (wg8: wg_pair_tile2<1>) and M = 4 (duo: wg_pair_tile2<2>)
ENDS_N = 200                                                  # four tiles: the pairs start at tile 2


def ends_lattice():
    """200 bodies on a jittered 6 x 6 lattice of layers (the construction of test_range_ends_of_the_staged_term), and their masses"""
    rng = np.random.default_rng(23)
    idx = np.arange(ENDS_N)
    pos = np.stack([idx % 6, (idx // 6) % 6, idx // 36], axis=1) + rng.uniform(-0.2, 0.2, size=(ENDS_N, 3))
    return pos, rng.uniform(1.0, 1e5, ENDS_N)


def all_n2(pos):
    d = pos[None, :, :] - pos[:, None, :]
    n2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return n2[~np.eye(len(pos), dtype=bool)]


def ends_cases(order):
    """(end, low, pos, mu, band): the lattice scaled so that the smallest n2 lies just above 2^-(end - 1), then so that the largest
    lies just below 2^(end - 1), at the order's own range end (2^+-300; 2^+-133 for order 5) -- with the conditions asserted: every
    n2 inside the guarded range, the band next to the end holding at least 1386 (low) and 13628 (high) operands"""
    pos0, mu = ends_lattice()
    n2 = all_n2(pos0)
    end = 133 if order >= 4 else 300
    out = []
    for f, low in ((np.sqrt(1.01 * 2.0 ** -(end - 1) / n2.min()), True), (np.sqrt(0.99 * 2.0 ** (end - 1) / n2.max()), False)):
        pos = pos0 * f
        v = all_n2(pos)
        assert v.min() >= 2.0 ** -end and v.max() < 2.0 ** end, ("outside the guarded range", order, end, low)
        if low:
            band = (v >= 2.0 ** -(end - 1)) & (v < 2.0 ** -(end - 3))
            assert 2.0 ** -(end - 1) <= v.min() < 2.0 ** -(end - 3), (order, end, np.log2(v.min()))
        else:
            band = (v > 2.0 ** (end - 3)) & (v <= 2.0 ** (end - 1))
            assert 2.0 ** (end - 3) < v.max() <= 2.0 ** (end - 1), (order, end, np.log2(v.max()))
        assert band.sum() >= (1386 if low else 13628), (order, end, low, band.sum())
        assert not ws.n2_out_of_range(v, order).any() and not fail_matrix(pos, mu, order).any(), ("the order's own range test", order, low)
        out.append((end, low, pos, mu, int(band.sum())))
    return out
