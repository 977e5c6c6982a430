"""Scenes for wave_force (csrc/step_wave.hip: the one-wave-per-block force of k_accel<BPW> and k_lm_step<BPW, L>) at the edges of its
tile walk, shared by tests/test_wave_scenes.py (CPU: every scene takes the branch it was planted for, on the restated walk and the
restated range test) and tests/test_gpu_wave_form.py (the kernels against the C oracle, bit pattern against bit pattern). A plain
module: no fixtures, no GPU import.

The walk. A wave carries the bodies i0 .. i0 + BPW - 1 (those past n - 1 are clamped copies of body n - 1) against the sources in tiles
of 64. With tiles = ceil(n / 64), tfull = n // 64 and d = i0 // 64 it visits

    run [0, min(d, tfull))   special(d)   and, where d < tfull:   run [d + 1, tfull)   special(tfull) if tfull < tiles

`special` is the un-pipelined tile (the wave's own bodies and / or the ragged last tile): IEEE arithmetic, no range test. A run [tb, te)
is the software pipeline: tile tb is its PROLOGUE (IEEE, no range test either), and tile tb + k, 1 <= k < te - tb, is finished in
step k - 1 of the run, in ping-pong phase (k - 1) & 1, behind ONE range test over the wave's BPW bodies and the tile's 64 sources.
Where that test fails the step takes its fallback branch: the IEEE term on the ping-pong registers, the hand-over of the next tile's
differences and mass, the un-interleaved chain. The step with k = te - tb - 1 is the run's last (nothing is handed over behind it).

What is planted (all at n = 330: tiles 0-4 whole, tile 5 ragged with 10 sources), and for what:

  near(s, body)   `body` at the origin, source s 2^-151 from it on every axis: n2 = 3 * 2^-302, below every order's guarded range, for
                  that pair alone. body 10 with s = 140, 200, 300: the upper run [1, 5) of body 10's wave in phase 0, phase 1 and
                  its last step (the reverse direction meets tile 0 as a prologue). body 300 with s = 70, 140, 200: the lower run
                  [0, 4) in phase 0, phase 1 and its last step.
  far(s)          source s at (2^151, 0, 0), body 10 at the origin: n2 ~ 2^302 for EVERY wave, and two zero components against
                  body 10. s = 140, 200, 300: one scene meets the run of every target tile at another position.
  massless(200)   mu[200] = 0: order 4 divides mu (order 5 takes a +0 mass on its fast sequence: its mu_key lets it pass).
  tiny_mass(200)  mu[200] = 1e-70, below 2^-200: orders 4 and 5. Tile 3 is a tested step for the targets of tiles 0, 1, 4 and 5.
  coincident      source 262 equal to body 5 in x and y: n2 in range, two component squares +0 -- orders 4 and 6 (low_key)."""
import numpy as np

TILE = 64
N = 330
ORDERS = (0, 4, 5, 6)
BPWS = (1, 2, 4, 8)
TILE_SIZES = (128, 129, 191, 192, 193, 256, 320, 383, 384, 385, 448, 449, 511, 512)
BPW_SIZES = (65, 130, 131, 197, 330, 705)
METHODS = {"QuinlanTremaine12": 12, "Stormer13": 13}          # method: L (ring length = start-up steps)
H = 1.0 / 1024.0

PROLOGUE, SPECIAL, STEP = "prologue", "special", "step"


# ---- the tile walk of wave_force, restated
def runs(n, i0):
    """the pipelined runs [tb, te) of the wave whose first body is i0, and the special tiles, in the order they are visited"""
    tiles, tfull, d = (n + TILE - 1) // TILE, n // TILE, i0 // TILE
    lower, specials, upper = (0, min(d, tfull)), [d], None
    if d < tfull:
        upper = (d + 1, tfull)
        if tfull < tiles:
            specials.append(tfull)
    return lower, upper, specials


def schedule(n, i0):
    """tile -> role: PROLOGUE, SPECIAL or (STEP, phase, last) -- the step in which the tile's range test is made"""
    lower, upper, specials = runs(n, i0)
    role = {t: SPECIAL for t in specials}
    for run in (lower, upper):
        if run is None or run[0] >= run[1]:
            continue
        tb, te = run
        role[tb] = PROLOGUE
        for k in range(1, te - tb):
            role[tb + k] = (STEP, (k - 1) & 1, k == te - tb - 1)
    return role


def run_of(i0, tile):
    """which run of the wave a stepped tile belongs to"""
    return "lower" if tile < i0 // TILE else "upper"


# ---- the range test of a step (csrc/pair_term.h: kRangeBase / kRangeSpan, range_key; kLowSq, low_key; mu_key; ieee_seq.h: in_range_div)
LOWSQ = 0x01700000                                            # high word of 2^-1000
DIV_BASE, DIV_SPAN = 0x33700000, 0x19000000                   # in_range_div: biased exponent in [823, 1223)


def range_consts(order):
    """(kRangeBase, kRangeSpan): biased exponent of n2 in [890, 1156) for the division forms, [723, 1323) otherwise"""
    return (0x37A00000, 0x10A00000) if order >= 4 else (0x2D300000, 0x25800000)


def hi_word(x):
    """__double2hiint as an unsigned word, elementwise"""
    return (np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


def n2_out_of_range(n2, order):
    base, span = range_consts(order)
    return ((hi_word(n2) - base) & 0xffffffff) >= span


def in_range_div(x):
    return ((hi_word(x) - DIV_BASE) & 0xffffffff) < DIV_SPAN


def mu_fails(mu, order):
    """mu_key != 0: orders 4 and 5 divide mu; order 5 lets a +0 through"""
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    if order == 4:
        return ~in_range_div(mu)
    if order == 5:
        return ~((mu.view(np.uint64) == 0) | in_range_div(mu))
    return np.zeros(mu.shape, dtype=bool)


def fail_matrix(pos, mu, order):
    """[i, j]: does the directed operand (target i, source j) fail the range test of a step. d = p_j - p_i, the three squares and
    n2 = (sx + sy) + sz are formed as pair_pre of pair_term.h forms them; the diagonal (never met by a step) is False"""
    pos, mu = np.asarray(pos, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    d = pos[None, :, :] - pos[:, None, :]
    s = d * d
    n2 = (s[..., 0] + s[..., 1]) + s[..., 2]
    bad = n2_out_of_range(n2, order) | mu_fails(mu, order)[None, :]
    if order in (4, 6):
        bad |= hi_word(s).min(axis=2) < LOWSQ
    bad[np.diag_indices(len(mu))] = False
    return bad


def failing_operands(pos, mu, order):
    """every directed operand (i, j), i != j, that fails the range test, wherever the walk meets it"""
    return [(int(i), int(j)) for i, j in np.argwhere(fail_matrix(pos, mu, order))]


def wave_bodies(n, i0, bpw):
    return sorted({min(i0 + b, n - 1) for b in range(bpw)})


def fallback_steps(pos, mu, order, bpw):
    """the set of (i0, tile, phase, last): the steps in which the wave of bodies i0 .. i0 + bpw - 1 fails its one-ballot range test"""
    bad = fail_matrix(pos, mu, order)
    n, out = len(bad), set()
    for i0 in range(0, n, bpw):
        rows = bad[wave_bodies(n, i0, bpw)]
        for tile, role in schedule(n, i0).items():
            if role in (PROLOGUE, SPECIAL):
                continue
            if rows[:, tile * TILE:(tile + 1) * TILE].any():   # a stepped tile is whole
                out.add((i0, tile, role[1], role[2]))
    return out


def wave_of(body, bpw):
    return body - body % bpw


# ---- scenes
class Scene:
    def __init__(self, name, pos, mu, orders, planted=()):
        """orders: the evaluation orders in which the scene leaves the range; planted: (body, tile, phase, last, run) that
        fallback_steps must contain for the wave of `body` in those orders"""
        self.name, self.pos, self.mu, self.orders, self.planted = name, pos, mu, tuple(orders), tuple(planted)


def base():
    """330 bodies ~1e7 apart, distinct mu in [1, 1e5], body 10 at the origin; and the row body 10 was drawn with"""
    rng = np.random.default_rng(330)
    pos, mu = rng.normal(size=(N, 3)) * 1e7, rng.uniform(1.0, 1e5, N)
    drawn = pos[10].copy()
    pos[10] = 0.0
    return pos, mu, drawn


def velocities():
    return np.random.default_rng(331).normal(size=(N, 3))


def _planted(body, s):
    role = schedule(N, body)[s // TILE]
    assert role not in (PROLOGUE, SPECIAL), (body, s, role)
    return (body, s // TILE, role[1], role[2], run_of(body, s // TILE))


def near(s, body=10):
    pos, mu, drawn = base()
    if body != 10:
        pos[10] = drawn
        pos[body] = 0.0
    pos[s] = 2.0 ** -151
    return Scene(f"near({s},{body})", pos, mu, ORDERS, [_planted(body, s)])


def far(s):
    pos, mu, _ = base()
    pos[s] = (2.0 ** 151, pos[10][1], pos[10][2])
    return Scene(f"far({s})", pos, mu, ORDERS, [_planted(10, s)])


def massless(s=200):
    pos, mu, _ = base()
    mu[s] = 0.0
    return Scene(f"massless({s})", pos, mu, (4,), [_planted(10, s), _planted(300, s)])


def tiny_mass(s=200):
    pos, mu, _ = base()
    mu[s] = 1e-70
    return Scene(f"tiny_mass({s})", pos, mu, (4, 5), [_planted(10, s), _planted(300, s)])


def coincident():
    pos, mu, _ = base()
    pos[262] = (pos[5][0], pos[5][1], pos[5][2] + 1e7)
    return Scene("coincident", pos, mu, (4, 6), [_planted(5, 262)])


NEAR_UPPER, NEAR_LOWER = (140, 200, 300), (70, 140, 200)


def near_scenes():
    return [near(s) for s in NEAR_UPPER] + [near(s, 300) for s in NEAR_LOWER]


def scenes():
    return near_scenes() + [far(140), far(200), far(300), massless(), tiny_mass(), coincident()]


def scene(name):
    return {s.name: s for s in scenes()}[name]


STEPPED = ("near(200,10)", "far(140)")                        # the scenes that are also stepped (QuinlanTremaine12, 12 + 3 steps)


# ---- comparisons
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differing_bodies(got, want):
    """indices of the bodies (rows) whose bit patterns differ"""
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))


def assert_same(got, want, what):
    bad = differing_bodies(got, want)
    if len(bad):
        b = int(bad[0])
        raise AssertionError(f"{what}: body {b} ({len(bad)} of {len(want)} bodies differ): {np.asarray(got)[b]} against "
                             f"{np.asarray(want)[b]}")


def assert_same_run(g, o, what):
    """an integration against its oracle: positions, velocities, time, step count, acc()"""
    gp, gv, gt, gc = g.state()
    op, ov, ot, oc = o.state()
    assert (gt, gc) == (ot, oc), f"{what}: (time, steps) {(gt, gc)} against {(ot, oc)}"
    assert_same(gp, op, f"{what}: positions")
    assert_same(gv, ov, f"{what}: velocities")
    assert_same(g.acc(), o.acc(), f"{what}: acc()")


def random_system(n, seed=0):
    """positions ~1e7, velocities ~1, distinct mu in [1, 1e5], seeded by (n, seed)"""
    rng = np.random.default_rng([n, seed])
    return rng.normal(size=(n, 3)) * 1e7, rng.normal(size=(n, 3)), rng.uniform(1.0, 1e5, size=n)


def stepped_system(n):
    """a Plummer sphere (positions and velocities ~1, so that a last bit of an acceleration reaches the state within a step) with
    DISTINCT masses: workloads.plummer's are all 1 / n, and the two directed halves of a pair could swap theirs unseen"""
    from ephemeris_explorer_amd.workloads import plummer
    pos, vel, mu = plummer(n)
    return pos, vel, mu * np.random.default_rng(n).uniform(0.5, 1.5, size=n)
