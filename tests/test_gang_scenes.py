"""CPU: the scenes of tests/gang_scenes.py on the C oracle alone. Conditions, not measurements: each scene still steps on the edge it was
planted for (tests/test_gpu_gang_edges.py compares the device with these very runs, so a scene that went quiet would check nothing)."""
import numpy as np
import pytest

import gang_scenes as gs
from oracle import orc
from wg_solout_scenes import trigger_period


@pytest.mark.parametrize("n", gs.SIZES)
def test_what_the_kernel_derives_from_the_size(n):
    """second pairs of the four-wave form, waves that hold owner threads, row length: the closed forms against the counts"""
    assert gs.live_second_pairs(n) == max(0, n * (n - 1) // 2 - 256)
    assert gs.owner_waves(n) == (6 * n - 1) // 64 + 1
    assert gs.row_length(n) == (n + 15) & ~15


def test_the_sizes_sit_on_both_sides_of_every_edge():
    assert gs.SIZES == (1, 2, 3, 10, 11, 16, 17, 21, 22, 23, 24, 25, 31, 32)
    assert [gs.live_second_pairs(n) for n in (23, 24, 25, 31, 32)] == [0, 20, 44, 209, 240]
    assert [gs.owner_waves(n) for n in (10, 11, 21, 22)] == [1, 2, 2, 3]
    assert [gs.row_length(n) for n in (16, 17)] == [16, 32]
    assert gs.npairs(1) == 0 and gs.npairs(2) == 1
    # 24, 25 and 31: live and dead second pairs inside one wave (a wave-uniform mistake in `live1` would pass 23 and 32)
    for n in (24, 25, 31):
        assert any(0 < sum(1 for lane in range(64) if 64 * w + lane + 256 < gs.npairs(n)) < 64 for w in range(4)), n


@pytest.mark.parametrize("sign", [1, -1])
def test_members_have_distinct_masses_and_one_massless_body(sign):
    for m in gs.edge_members(sign):
        assert m.h == sign * 60.0 and m.pos.shape == (m.n, 3)
        assert len(set(m.mu.tolist())) == m.n                                       # no two alike: vi.w for vj.w shows
        assert (m.mu == 0.0).sum() == (1 if sign < 0 else 0)
        live = m.mu[m.mu != 0.0]
        assert ((live >= 1.0) & (live <= 1e5)).all()
        assert 1e5 < np.abs(m.pos).max() < 1e8 and np.abs(m.vel).max() < 10.0
    assert np.array_equal(gs.edge_member(17, 1).pos, gs.edge_member(17, 1).pos)      # seeded by n


def test_pair_index_is_the_kernels_decode():
    """small_decode (small_frame.h), restated: q -> (i, j), against pair_index"""
    for n in gs.SIZES:
        q = 0
        for i in range(n):
            for j in range(i + 1, n):
                assert gs.pair_index(i, j, n) == q
                q += 1
        assert q == gs.npairs(n)
    assert gs.far_pair_index(False) == 264 and gs.far_pair_index(True) == 0
    assert 264 - gs.PAIR_THREADS_TWO == 8                                           # second pair of lane 8 of wave 0


FAR_STEPS = 100        # more than any handle of tests/test_gpu_gang_edges.py takes on a far-pair scene: L + (L - 1) + sum(gang_calls(L)) <= 89


@pytest.mark.parametrize("method", list(gs.METHODS))
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("variant", [0, 4])
def test_far_pair_scene_keeps_exactly_one_pair_out_of_range(method, mirrored, variant):
    """on the oracle's states, at the start and after every step: one out-of-range pair, index 264 (mirrored: 0); the state stays
    finite and the far body's acceleration is a normal double"""
    E = gs.range_exponent(variant)
    assert E == (300 if variant == 0 else 133)
    m = gs.far_pair(E, mirrored)
    want = [gs.far_pair_index(mirrored)]
    assert gs.out_of_range_pairs(m.pos, E) == want
    far = (0, 1) if mirrored else (gs.FAR_I, gs.FAR_J)
    # how far out it is: below 2^(E + 2), and no scene can do better for a second pair ALONE -- every body is some first pair's
    # partner of a body of the same wave, so both ends are within 2^(E / 2) of that body (profiles/gang_edges.md, change (b))
    d = m.pos[far[1]] - m.pos[far[0]]
    assert 2.0 ** E <= d @ d < 2.0 ** (E + 2)
    near = [b for b in range(32) if b not in far]
    assert np.abs(m.pos[near]).max() < 1e8 and (m.vel[list(far)] == 0.0).all()
    assert (m.pos[list(far), 1:] != 0.0).all() and m.pos[far[0], 0] == -m.pos[far[1], 0] == -0.99 * 2.0 ** (E / 2)
    orc.set_pair_variant(variant)
    try:
        o = m.make(orc.NBody, method)
        for s in range(FAR_STEPS):
            assert o.advance(1) == 0
            pos, vel, _, _ = o.state()
            assert gs.out_of_range_pairs(pos, E) == want, (s, gs.out_of_range_pairs(pos, E))
            assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(o.acc()).all()
        a = np.abs(o.acc()[far[0]]).max()
    finally:
        orc.set_pair_variant(0)
    assert a > 2.3e-308                                                              # normal: nothing is flushed on the way
    if variant == 0:
        assert 1e-85 < a < 1e-83, a                                                  # ~8e-85: sum of mu / X^2


@pytest.mark.parametrize("method", list(gs.METHODS))
def test_desynchronised_gang_enters_with_many_ring_slots(method):
    """arithmetic, and the oracle's own step counts through run_gang: at every ganged call at least five ring positions"""
    L = gs.METHODS[method]
    assert gs.gang_calls(L) == (1, 5, L, L + 1, 2 * L + 5)
    members = gs.edge_members(1)
    slots = gs.entry_slots(len(members), L)
    assert len(slots) == 5 and all(len(set(s)) >= 5 for s in slots), slots
    _, rec = gs.run_gang(members, method, orc.NBody)
    assert len(rec) == 6
    done = 0
    for c, k in enumerate((0,) + gs.gang_calls(L)):
        done += k
        steps = [int(r["steps"][0]) for r in rec[c]]
        assert steps == [L + gs.desync_steps(i, L) + done for i in range(len(members))]
        if c < 5:
            assert [s % L for s in steps] == slots[c]
        assert all(r["t"][0] == 60.0 * s for r, s in zip(rec[c], steps))
    # the shared oracle of the GPU file (one step at a time, kept) gives the bits of the advance(k) calls
    gs.compare_gang(members, gs.expected_gang(members, method, gs.Oracle()), rec, "trail against advance(k)")
    # a gang padded with clones to more handles than a chip has CUs: every (source, steps alone) of a clone occurs at least twice,
    # the sources enter as above, and the clones add ring positions of their own
    sources = 2 * len(members) + 2
    plan = gs.padded_plan(sources, 264, L)
    assert plan[:len(members)] == [(i, L + gs.desync_steps(i, L)) for i in range(len(members))]
    clones = plan[sources:]
    assert len(plan) == 264 and all(clones.count(key) >= 2 for key in clones) and {src for src, _ in clones} == set(range(sources))
    assert {alone - plan[src][1] for src, alone in clones} == {1, 2, 3}
    assert len({alone % L for _, alone in plan}) == L


@pytest.mark.parametrize("method", list(gs.METHODS))
def test_sampled_gang_completes_windows_and_enters_in_mid_period(method):
    L = gs.METHODS[method]
    members = gs.sampled_members()
    assert [m.n for m in members] == [1, 1, 3, 3, 17, 17, 24, 24, 32, 32] and {m.direction for m in members} == {1, -1}
    entries = [m.entry_steps(L) for m in members]
    assert len(set(entries)) == len(entries) and min(entries) > L and len({e % L for e in entries}) >= 5, entries
    ganged = sum(gs.SAMPLED_CALLS)
    rec, _ = gs.run_sampled(members, method, orc.Propagator)
    for m, e, r in zip(members, entries, rec):
        period = np.array([trigger_period(gs.H, int(c)) for c in m.count])
        assert np.array_equal(period, m.count.astype(np.int64))                      # 60 s accumulate exactly: every body samples
        assert int(r["steps"][0]) == e + ganged
        for b in range(m.n):
            window = gs.KDIV * int(period[b])
            assert (e + ganged) // window > e // window, (m.name, b)                  # a window ends inside the ganged steps
        assert np.array_equal(r["npoly"], (e + ganged) // (gs.KDIV * period))         # and was fitted and handed over
        phases = {int(e % c) for c in m.count} - {0}
        if m.n >= 3:
            assert len(phases) >= 2, (m.name, e, phases)
    assert {int(d) for m in members for d in m.degree} == {2, 3, 4, 5, 6, 7}
    assert {int(c) for m in members for c in m.count} == {1, 2, 3, 7, 12}


def test_the_comparisons_name_what_differs():
    """what the GPU file relies on: equal runs pass, one flipped bit is found and named"""
    members = gs.edge_members(-1)[:4]
    _, rec = gs.run_gang(members, "QuinlanTremaine12", orc.NBody)
    gs.compare_gang(members, rec, rec, "self")
    bad = [[dict(r) for r in call] for call in rec]
    acc = bad[3][2]["acc"].copy()
    acc[1, 2] = np.nextafter(acc[1, 2], np.inf)
    bad[3][2]["acc"] = acc
    with pytest.raises(AssertionError, match=r"flipped: after ganged call 2, member n3-: acc of body 1 "):
        gs.compare_gang(members, bad, rec, "flipped")
    sm = gs.sampled_members()[2:4]
    srec, _ = gs.run_sampled(sm, "Stormer13", orc.Propagator)
    gs.compare_sampled(sm, srec, srec, "self")
    sbad = [dict(r) for r in srec]
    co = sbad[1]["coef"].copy()
    q = int(np.cumsum(srec[1]["npoly"])[1])                                          # body 2's first polynomial
    co[q, 0, 1] = np.nextafter(co[q, 0, 1], np.inf)
    sbad[1]["coef"] = co
    with pytest.raises(AssertionError, match=rf"flipped: member p3-: coef of polynomial {q} of the take \(body 2, count 3, degree 4\)"):
        gs.compare_sampled(sm, sbad, srec, "flipped")
