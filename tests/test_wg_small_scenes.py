"""CPU: the scenes of tests/wg_small_scenes.py on the restated schedule of the 4-body, twelve-wave 8-body and six-wave 8-body (duo)
workgroup forms of csrc/step_wg.hip, and on the C oracle. Conditions, not measurements: each scene still reaches the unit, the tile
and the branch it was planted for (tests/test_gpu_wg_small_forms.py compares the device with the oracle on these very scenes, so a
scene that went quiet would check nothing), and the quiet steps that file takes keep it there."""
from fractions import Fraction

import numpy as np
import pytest

import wave_scenes as ws
import wg_small_scenes as wg
from oracle import orc

SCENES = {s.name: s for s in wg.scenes()}
NAMES_330 = ["near(140,10)", "near(200,10)", "near(300,10)", "near(325,10)", "near(200,11)", "near(200,301)", "near(70,300)",
             "near(20,300)", "near(329,10)", "far(200)", "far(329)", "far(201,2^400)", "far(140,2^400)", "massless(140)",
             "massless(200)", "massless(325)", "tiny_mass(140)", "tiny_mass(200)", "tiny_mass(325)", "coincident(262,5)",
             "coincident(200,5)", "faint_tile(3)", "thin_tile(3)"]
NAMES_280 = ["near(270,10)@280", "far(279)@280", "far(271,2^400)@280"]
NAMES_NATURAL = [f"{s}@{n}" for n in (600, 1100)
                 for s in ("near(200,10)", f"near({n - 5},10)", f"far({n - 1})", "tiny_mass(350)", "far(201,2^400)")]
ISOLATING = {"faint_tile(3)": 5, "thin_tile(3)": 6}         # scene: the order in which ONLY the units holding its tile matter
OVERFLOWING = ["far(201,2^400)", "far(140,2^400)", "far(271,2^400)@280", "far(201,2^400)@600", "far(201,2^400)@1100"]


def test_big_tiles_are_the_kernels():
    """big_start(K) = K < 2 ? K : 2 K - 2, big_count(tiles) = tiles <= 2 ? tiles : 2 + (tiles - 1) / 2, and `produce` taking
    wg_pair_tile2 when K >= 2 and the second tile exists: read off for tiles = 1 .. 7"""
    assert [wg.big_tiles(t) for t in range(1, 8)] == [
        [(0,)],
        [(0,), (1,)],
        [(0,), (1,), (2,)],
        [(0,), (1,), (2, 3)],
        [(0,), (1,), (2, 3), (4,)],
        [(0,), (1,), (2, 3), (4, 5)],
        [(0,), (1,), (2, 3), (4, 5), (6,)]]
    for tiles in range(1, 40):                              # every tile once, in order
        assert [t for g in wg.big_tiles(tiles) for t in g] == list(range(tiles))


def test_the_units_of_a_launch():
    """n = 330: 83 workgroups of 4 bodies x 6 tiles, 42 of 8 bodies x 4 big tiles, 42 x 4 two-body waves x 4 big tiles; the last
    workgroup's bodies past 329 are copies of it; a unit with the workgroup's own tile is not tested; the lanes of the ragged tile"""
    count = {form: len(list(wg.units(330, form))) for form in wg.FORMS}
    assert count == {"wg4": 83 * 4 * 6, "wg8": 42 * 8 * 4, "duo": 42 * 4 * 4}
    last = {form: [u for u, _ in wg.units(330, form) if u.i0 == 328 and u.tiles[0] == 0] for form in wg.FORMS}
    assert [u.bodies for u in last["wg4"]] == [(328,), (329,), (329,), (329,)]
    assert [u.bodies for u in last["wg8"]] == [(328,)] + [(329,)] * 7
    assert [u.bodies for u in last["duo"]] == [(328, 329)] + [(329, 329)] * 3
    for form in wg.FORMS:
        for u, tested in wg.units(330, form):
            assert tested == (u.i0 // 64 not in u.tiles)
    assert wg.lane_sources(330, 5).tolist() == list(range(320, 330)) + [329] * 54
    assert wg.lane_sources(330, 4).tolist() == list(range(256, 320))
    assert [wg.position(330, t, "wg8") for t in range(6)] == [(wg.SINGLE, False), (wg.SINGLE, False), (wg.FIRST, False),
                                                               (wg.SECOND, False), (wg.FIRST, False), (wg.SECOND, True)]
    assert wg.position(280, 4, "duo") == (wg.SINGLE, True) and wg.position(330, 5, "wg4") == (wg.SINGLE, True)
    assert wg.position(600, 9, "wg8") == (wg.SECOND, True) and wg.position(1100, 17, "duo") == (wg.SECOND, True)


def test_the_scenes_are_the_ones_asked_for():
    assert list(SCENES) == NAMES_330 + NAMES_280 + NAMES_NATURAL
    assert wg.STORMER in NAMES_330 and set(wg.NATURAL_SIZES) == {600, 1100}
    where = {name: SCENES[name].where for name in SCENES}
    assert [where[f"near({s},10)"] for s in (140, 200, 300, 325)] == [(wg.FIRST, False), (wg.SECOND, False), (wg.FIRST, False),
                                                                      (wg.SECOND, True)]
    assert where["near(70,300)"] == where["near(20,300)"] == (wg.SINGLE, False)
    assert [where[f"{k}({s})"] for k in ("massless", "tiny_mass") for s in (140, 200, 325)] == [
        (wg.FIRST, False), (wg.SECOND, False), (wg.SECOND, True)] * 2
    assert where["coincident(262,5)"] == (wg.FIRST, False) and where["coincident(200,5)"] == (wg.SECOND, False)
    assert where["near(270,10)@280"] == where["far(279)@280"] == (wg.SINGLE, True)
    for n in (600, 1100):
        assert [where[f"{s}@{n}"] for s in ("near(200,10)", f"near({n - 5},10)", f"far({n - 1})", "tiny_mass(350)")] == [
            (wg.SECOND, False), (wg.SECOND, True), (wg.SECOND, True), (wg.SECOND, False)]
        assert (350 // 64) % 2 == 1
    for s in (140, 200, 325):
        assert SCENES[f"massless({s})"].mu[s] == 0.0 and SCENES[f"tiny_mass({s})"].mu[s] == 1e-70
        assert SCENES[f"massless({s})"].orders == (4,) and SCENES[f"tiny_mass({s})"].orders == (4, 5)
    for name in ("coincident(262,5)", "coincident(200,5)"):
        c, s = SCENES[name], int(name[11:14])
        d = c.pos[s] - c.pos[5]
        assert c.orders == (4, 6) and d[0] == 0.0 and d[1] == 0.0 and d[2] == 1e7
    for name in ("far(200)", "far(329)", "far(279)@280", "far(599)@600", "far(1099)@1100"):
        f, s = SCENES[name], int(name[4:name.index(")")])
        d = f.pos[s] - f.pos[10]
        assert (d == (2.0 ** 151, 0.0, 0.0)).all() and (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == 2.0 ** 302
    assert [where[name] for name in OVERFLOWING] == [(wg.SECOND, False), (wg.FIRST, False), (wg.SINGLE, True), (wg.SECOND, False),
                                                     (wg.SECOND, False)]


@pytest.mark.parametrize("name", OVERFLOWING)
def test_the_overflowing_source_keeps_every_result_finite(name):
    """a source 2^400 away: n2 = 2^800 is finite, p = n2 sqrt(n2) is not, and the IEEE term is +0 in every order -- every acceleration
    of the scene is finite, the far body's own is exactly zero. (On the wrapper-free sequences q = h h h 8 underflows to 0 beside
    p = inf and e = fma(-p, q, 1) is NaN: a unit that took the fast branch with this operand would not return these bits.) As a
    BODY, source 201 is the second of its duo wave, and 200 beside it stays in range against the tiles 0 and 1"""
    sc = SCENES[name]
    body, s = sc.planted[0]
    d = sc.pos[s] - sc.pos[body]
    n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    with np.errstate(over="ignore"):
        assert n2 == 2.0 ** 800 and np.isinf(n2 * np.sqrt(n2)) and 1.0 / (n2 * np.sqrt(n2)) == 0.0
    try:
        for order in range(7):
            orc.set_pair_variant(order)
            a = orc.gravity(sc.pos, sc.mu)
            assert np.isfinite(a).all() and (a[s] == 0.0).all() and (np.delete(a, s, axis=0) != 0.0).all(), (name, order)
    finally:
        orc.set_pair_variant(0)
    if s == 201:
        u = wg.unit_of(sc.n, "duo", 201, 0)
        bad = wg.operand_fails(sc.pos, sc.mu, 0)
        assert u.bodies == (200, 201) and u.tiles == (0,) and bad[201, :64].all() and not bad[200, :64].any()


@pytest.mark.parametrize("n", [330, 280, 600, 1100])
def test_the_base_systems_never_leave_the_range(n):
    pos, mu, _ = wg.system(n)
    assert len(set(mu.tolist())) == n and mu.min() >= 1.0 and mu.max() <= 1e5 and (pos[10] == 0.0).all()
    for order in range(7):
        assert not ws.fail_matrix(pos, mu, order).any()


def near_expected(sc, form):
    """the two directed halves of a near pair; where the source is the clamp body n - 1, the last workgroup's copies of it as well"""
    (body, s), n = sc.planted[0], sc.n
    want = {wg.unit_of(n, form, body, s // 64), wg.unit_of(n, form, s, body // 64)}
    if s == n - 1:
        want |= {u for u, _ in wg.units(n, form) if s in u.bodies and body // 64 in u.tiles}
    return want


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("order", wg.ORDERS)
def test_scene_reaches_the_unit_it_was_planted_for(name, order):
    """every form: in the orders the scene names, the planted operand's unit fails its ballot, through the tile it was planted in
    (first / second / single, ragged or whole); in the other orders nothing fails anywhere. A near scene fails exactly the units
    of its two directed halves (fast and slow units in one launch); a far source, a massless or a tiny one fails the unit holding
    its tile for every workgroup. A failing unit of wg_pair_tile2 holds at least 64 operands that pass the range test: their terms
    go through the IEEE form as well, which must give them the same bits. (The one exception is stated, not filtered: the units
    whose only body is the far body ITSELF -- on wg8, and the clamped copies of a far last body on duo -- are 2^151 away from all 128
    sources and have no operand in range. For faint_tile and thin_tile, where whole systems are out of range by construction, it is
    asserted for the planted unit in the order that isolates the tile.)"""
    sc = SCENES[name]
    bad = wg.operand_fails(sc.pos, sc.mu, order)
    for form in wg.FORMS:
        got = wg.failing_units_of(bad, form)
        assert got == wg.failing_units(sc, order, form)
        if order not in sc.orders:
            assert got == {} and not ws.fail_matrix(sc.pos, sc.mu, order).any(), (name, order, form)
            continue
        tested = [u for u, t in wg.units(sc.n, form) if t]
        for body, s in sc.planted:
            u = wg.unit_of(sc.n, form, body, s // 64)
            assert body in u.bodies and s // 64 in got[u], (name, order, form, body, s)
            assert ws.fail_matrix(sc.pos, sc.mu, order)[body, s]
        body, s = sc.planted[0]
        u = wg.unit_of(sc.n, form, body, s // 64)
        expect = (wg.SINGLE, sc.where[1]) if form == "wg4" else sc.where
        assert wg.position(sc.n, s // 64, form) == expect and len(u.tiles) == (1 if expect[0] == wg.SINGLE else 2)
        if expect[0] != wg.SINGLE:
            assert u.tiles.index(s // 64) == (expect[0] == wg.SECOND)
        if name.startswith("near"):
            assert set(got) == near_expected(sc, form) and len(got) < len(tested), (name, order, form)
            assert sorted(ws.failing_operands(sc.pos, sc.mu, order)) == sorted([(body, s), (s, body)])
            d = sc.pos[s] - sc.pos[body]
            assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == 3 * 2.0 ** -302
            if name == "near(329,10)":
                assert len(got) == {"wg4": 4, "wg8": 8, "duo": 5}[form]
            else:
                assert len(got) == 2
            if form == "duo" and body in (11, 301):         # the second body of its wave alone carries the operand
                assert u.bodies == (body - 1, body) and not bad[body - 1, wg.lane_sources(sc.n, s // 64)].any()
                assert not bad[body - 1, np.concatenate([wg.lane_sources(sc.n, t) for t in u.tiles])].any()
        elif name.startswith("coincident"):
            assert set(got) == {wg.unit_of(sc.n, form, body, s // 64), wg.unit_of(sc.n, form, s, body // 64)}
        else:                                               # far, massless, tiny_mass: every workgroup's unit with the tile
            holding = [v for v in tested if s // 64 in v.tiles]
            if name.startswith("thin"):                     # (the partner tile's own bodies are 2^-400 from tile 3 in x: they pass)
                holding = [v for v in holding if v.i0 // 64 != s // 64 - 1]
            assert len(holding) >= (sc.n - 128) // (2 if form == "duo" else 1) and all(s // 64 in got[v] for v in holding)
            if name in ISOLATING:
                # the order that isolates the tile: the unit fails through that tile alone (its partner's operands pass); faint:
                # no other unit fails. In the scene's other order (4: the +0 masses) every tested unit fails
                if order == ISOLATING[name]:
                    assert all(got[v] == (s // 64,) for v in holding) and (name.startswith("thin") or set(got) == set(holding))
                else:
                    assert order == 4 and (name.startswith("thin") or set(got) == set(tested))
            elif not name.startswith("far"):
                assert set(got) == set(holding)
        far_source = s if name.startswith("far") else -1
        for v in ([u] if name in ISOLATING else got):
            if len(v.tiles) == 2 and set(v.bodies) != {far_source} and ISOLATING.get(name, order) == order:
                assert wg.in_range_operands(bad, v) >= 64, (name, order, form, v)


def fast_and_ieee_terms(sc, order, body, j):
    """the directed term (body <- source j) by the wrapper-free division step of csrc/pair_term.h, on the correctly rounded
    reciprocal q = RN(1 / p) that inv_r3_seeded is proved to return, in EXACT arithmetic (a Fraction converts to the nearest double),
    and by IEEE division -- orders 4, 5, 6"""
    rn = float
    d = sc.pos[j] - sc.pos[body]
    s = d * d
    n2 = (s[0] + s[1]) + s[2]
    p = n2 * np.sqrt(n2)
    mu = sc.mu[j]
    P, Q = Fraction(p), Fraction(rn(1 / Fraction(p)))

    def quotient(a):                                        # t = RN(a q); e = RN(a - p t) (one fma); RN(t + e q) (one fma)
        t = rn(Fraction(a) * Q)
        e = rn(Fraction(a) - P * Fraction(t))
        return rn(Fraction(t) + Fraction(e) * Q)
    if order == 4:
        return np.array([quotient(c * mu) for c in d]), np.array([(c * mu) / p for c in d])
    if order == 5:
        return d * quotient(mu), d * (mu / p)
    return np.array([quotient(c) * mu for c in d]), np.array([(c / p) * mu for c in d])


@pytest.mark.parametrize("name, order, least", [("faint_tile(3)", 5, 16), ("faint_tile(3)", 4, 16), ("thin_tile(3)", 6, 8),
                                                ("tiny_mass(200)", 4, 0), ("tiny_mass(200)", 5, 0), ("massless(200)", 4, 0),
                                                ("coincident(200,5)", 4, 0), ("coincident(200,5)", 6, 0), ("near(200,10)", 4, 0),
                                                ("near(200,10)", 5, 0), ("near(200,10)", 6, 0), ("far(200)", 4, 0),
                                                ("far(200)", 5, 0), ("far(200)", 6, 0)])
def test_which_scenes_a_wrongly_taken_fast_branch_would_show_in(name, order, least):
    """The guarded ranges are round guards, not the edge of validity: on the operands of the near, far, massless, tiny_mass and
    coincident scenes the wrapper-free quotient IS the IEEE quotient (least = 0: not one of the 64 terms of the planted unit's tile
    differs, bit for bit; a -0 against a +0 does not count, the sums absorb it), so those scenes hold the slow branch and the code
    behind it, but a unit that skipped its range test would return the same bits. faint_tile and thin_tile are the scenes such a
    unit shows in: the residual of the division step underflows for a subnormal numerator, and at least `least` of the 64 terms
    of body 10 against tile 3 come out different (far(s, 2^400) is the third: NaN against +0)"""
    sc = SCENES[name]
    body, s = sc.planted[0]
    differing = 0
    for j in wg.lane_sources(sc.n, s // 64):
        fast, ieee = fast_and_ieee_terms(sc, order, body, int(j))
        assert np.isfinite(fast).all() and np.isfinite(ieee).all()
        differing += not np.array_equal((fast + 0.0).view(np.uint64), (ieee + 0.0).view(np.uint64))   # (+ 0.0: -0 becomes +0)
    assert differing >= least and (least > 0 or differing == 0), (name, order, differing)


def test_the_clamped_copies_of_a_far_last_body_fail_too():
    """far(329): the padding lanes of tile 5 carry the out-of-range copy (54 of its 64 lanes), and the last workgroup's copies of
    body 329 fail against every tile they are tested on"""
    sc = SCENES["far(329)"]
    bad = wg.operand_fails(sc.pos, sc.mu, 0)
    assert bad[10, wg.lane_sources(330, 5)].sum() == 55
    for form in wg.FORMS:
        got = wg.failing_units_of(bad, form)
        copies = [u for u, t in wg.units(330, form) if t and u.i0 == 328 and 329 in u.bodies]
        assert copies and all(u in got and got[u] == u.tiles for u in copies), form


def stepped_cases():
    """(scene, order, method) of every quiet run tests/test_gpu_wg_small_forms.py makes"""
    out = [(name, order, "QuinlanTremaine12") for name in NAMES_330 + NAMES_280 for order in wg.ORDERS]
    out += [(wg.STORMER, order, "Stormer13") for order in wg.ORDERS]
    out += [(name, order, "QuinlanTremaine12") for name in NAMES_NATURAL for order in wg.NATURAL_ORDERS]
    return out


@pytest.mark.parametrize("name, order, method", stepped_cases())
def test_the_quiet_steps_keep_the_scene_where_it_was_planted(name, order, method):
    """t0 = 0, h = 2^-400, zero velocities: after L and after L + 3 steps the oracle's positions fail exactly the units the initial
    positions fail, in every form, so the fused step kernels meet the planted unit; everything is finite, and the velocities are
    not all zero (they carry the accelerations' bits)"""
    sc, L = SCENES[name], wg.METHODS[method]
    orc.set_pair_variant(order, native=True)
    try:
        o = orc.NBody(sc.pos, wg.zero_velocities(sc.n), sc.mu, 0.0, wg.QUIET_H, method, native=True)
        first = wg.operand_fails(sc.pos, sc.mu, order)
        for steps in (L, 3):
            assert o.advance(steps) == 0
            pos, vel, _, _ = o.state()
            assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(o.acc()).all()
            assert (o.acc() != 0.0).any() and (vel != 0.0).any() != sc.still   # (a still scene: acc() alone carries the bits)
            now = wg.operand_fails(pos, sc.mu, order)
            assert np.array_equal(now, first), (name, order, method)
            for form in wg.FORMS:
                assert wg.failing_units_of(now, form) == wg.failing_units_of(first, form)
        assert o.state()[3] == L + 3
    finally:
        orc.set_pair_variant(0, native=True)


def test_the_quiet_step_is_needed():
    """at h = 1 / 1024 the near pair's mutual acceleration throws it apart in the start-up: the scene then fails for every unit like
    a far one, and no longer has fast and slow units side by side"""
    sc = SCENES["near(200,11)"]
    o = orc.NBody(sc.pos, wg.zero_velocities(sc.n), sc.mu, 0.0, ws.H, native=True)
    assert o.advance(12) == 0
    assert len(wg.failing_units(sc, 0, "duo", o.state()[0])) > 2


@pytest.mark.parametrize("order", [0, 5])
def test_range_ends_lattice(order):
    """the band conditions of the range-end runs (asserted inside ends_cases), and that the lattice's 200 bodies put tested units of
    wg_pair_tile2 in front of the staged term: four tiles, the pair {2, 3}, tested for the 128 bodies of tiles 0 and 1"""
    cases = wg.ends_cases(order)
    assert [(end, low) for end, low, *_ in cases] == [(133 if order == 5 else 300, True), (133 if order == 5 else 300, False)]
    assert wg.big_tiles(wg.tile_count(wg.ENDS_N)) == [(0,), (1,), (2, 3)]
    for form, per in (("wg8", 1), ("duo", 2)):
        pairs = [u for u, t in wg.units(wg.ENDS_N, form) if t and len(u.tiles) == 2]
        assert len(pairs) == 128 // per
    orc.set_pair_variant(order)
    orc.set_pair_variant(order, native=True)
    try:
        for _, _, pos, mu, _ in cases:
            a = orc.gravity(pos, mu)
            assert np.isfinite(a).all() and (np.abs(a[a != 0]) >= 2.0 ** -1022).all()
            # the duo form meets the lattice in its fused step only: 12 + 3 quiet steps leave every position where it was
            o = orc.NBody(pos, wg.zero_velocities(wg.ENDS_N), mu, 0.0, wg.QUIET_H, native=True)
            for steps in (12, 3):
                assert o.advance(steps) == 0
                p, v, _, _ = o.state()
                assert np.array_equal(p, pos) and np.isfinite(v).all() and (v != 0.0).all() and np.isfinite(o.acc()).all()
    finally:
        orc.set_pair_variant(0)
        orc.set_pair_variant(0, native=True)


def test_the_comparison_names_what_differs():
    sc = SCENES["far(200)"]
    a = orc.gravity(sc.pos, sc.mu)
    wg.assert_same(a, a.copy(), "self")
    b = a.copy()
    b[201, 2] = np.nextafter(b[201, 2], np.inf)
    with pytest.raises(AssertionError, match=r"flipped: body 201 \(1 of 330 bodies differ\)"):
        wg.assert_same(b, a, "flipped")
