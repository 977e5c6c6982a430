"""-m gpu: eph_craft_batch_gather (csrc/craft_gather.hip, csrc/gather_plan.h): a batch built out of chosen craft of existing batches goes
on bit for bit like the craft it was built from. No tolerance anywhere: status, counters, every knot, the state, next_h and every
transition and apsis of every output craft, against the C oracle's single run of the craft it came from (orc.Craft) AND against the
source batch given the same later calls.

The material is scene T of tests/event_scenes.py (136 craft, semi-major axes over a factor 40, nested planted spheres, a different
history per craft: the smallest shape at which a deal to the lanes exists), in the pattern propagate to 0.4 T_END, gather, propagate to
T_END. Its preconditions -- the first leg finds some but not all events, the knot counts differ by more than a factor 2 -- hold on the
oracle alone (gather_preconditions; tests/test_craft_gather_scene.py asserts them without a GPU).

Wave forms in this process; the three thread forms (k_craft_propagate dealt, undealt, k_craft_queue) in one child process each (the
form is read once per process; this file run as a script), every child under its own timeout; after a child that died of a signal or
ran into its timeout the remaining children are not started. The commit rule runs in a child on the test-hooks library
(eph_debug_fail_alloc: a host function returns an error code, no fault is provoked), and so do its three siblings for the calls that
share the gather's statement of the batch's buffers (csrc/craft_batch.h): create, clone and enable_events. Each of the four also asserts
how many device allocations its call makes (ALLOCATIONS): a buffer dropped from, or added to, a walk over the statement moves a count."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import event_scenes as evs
from conftest import ROOT
from craft_cases import bits, same
from hooks import failing_allocations
from oracle import orc
from test_gpu_craft_events import DRAINED, SCENES, compare_events, compare_sweep, oracle_results
from test_gpu_live_ephemeris import DAY, _compare, _fleet, _live, _ship, pieces  # noqa: F401  (pieces: the fixture)

pytestmark = pytest.mark.gpu

METHOD = "Verner87"
FSAL_METHOD = "DormandPrince54"
HOOKS_LIB = ROOT / "ephemeris_explorer_amd" / "libephemeris_amd_testhooks.so"
KNOTS_FULL = 6
FORMS = ["thread-static", "thread-static-undealt", "thread-queue"]
_dead_children = []


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def gather_preconditions(method):
    """on the oracle alone: at 0.4 T_END some but not all events have been found, and the craft's knot counts differ by more than 2x"""
    sc = SCENES[f"T-{method}"]
    res, lists = oracle_results(sc.name, method)
    cut = 0.4 * sc.calls[-1][1]
    early = sum(int(np.count_nonzero(np.asarray(l[0][0]) <= cut)) + int(np.count_nonzero(np.asarray(l[1][0]) <= cut)) for l in lists)
    total = sum(len(l[0][0]) + len(l[1][0]) for l in lists)
    assert 0 < early < total, (early, total)
    nk = np.array([len(r["craft"].knots()[0]) for r in res])
    assert nk.max() >= 2 * nk.min() and nk.min() >= 2, (nk.min(), nk.max())
    return sc, res, lists


def params_of(ea, sc):
    p = sc.params
    return ea.AdaptiveParams(p["h_init"], p["h_max"], p["tol_pos"], p["tol_vel"], 1.0 / 5.0, 5.0 / 1.0, 9.0 / 10.0, 1_000_000)


def batch_of(ea, eph, sc, method, craft, events=True, params=None, burns=None, max_knots=None, max_tr=None, max_ap=None, soi=None):
    """the scene's craft `craft` (scene indices, any order, repeats allowed) as a batch on the shared table `eph`"""
    craft = np.asarray(craft, dtype=np.int64)
    b = ea.SpacecraftBatch(eph, sc.t0[craft], sc.pos[craft].reshape(-1, 3), sc.vel[craft].reshape(-1, 3), method, params or params_of(ea, sc),
                           [burns[i] for i in craft] if burns is not None else [sc.burns[i] for i in craft],
                           max_knots=max_knots or sc.max_knots)
    if events:
        b.enable_events(sc.soi if soi is None else soi, max_transitions=max_tr or sc.max_tr, max_apsides=max_ap or sc.max_ap)
    return b


def raw_gather(ea, sources, source_of, craft_of, n_out=None):
    """the C call itself -> (status, *out as an int or None, eph_last_error)"""
    handles = (C.c_void_p * len(sources))(*[s._h for s in sources])
    so = None if source_of is None else np.ascontiguousarray(source_of, dtype=np.int32)
    co = None if craft_of is None else np.ascontiguousarray(craft_of, dtype=np.int64)
    n = n_out if n_out is not None else (len(co) if co is not None else sum(s.n for s in sources))
    out = C.c_void_p(0x5A5A5A5A)
    st = ea._lib().eph_craft_batch_gather(len(sources), handles, n, None if so is None else so.ctypes.data_as(C.POINTER(C.c_int32)),
                                          None if co is None else co.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(out))
    return st, out.value, ea._lib().eph_last_error().decode()


def readable(b, events=True):
    """everything the ABI lets a caller read of a batch, per craft: summary records, used knots, event lists"""
    rec = b.summary()
    nk = rec["nknots"].astype(np.int64)
    rows = int(nk.max()) if b.n else 0
    t, y = b.knot_slabs(0, rows) if rows else (np.zeros((0, b.n)), np.zeros((0, 6, b.n)))
    out = dict(rec=rec, nk=nk, t=t, y=y)
    if events:
        counts = b.event_counts()
        out["counts"] = counts
        out["events"] = [b.events(i, counts) for i in range(b.n)]
    return out


def same_craft(a, i, b, j, what, events=True):
    """craft i of readable() `a` is bit for bit craft j of readable() `b`"""
    assert a["rec"][i].tobytes() == b["rec"][j].tobytes(), f"{what}: summary record {a['rec'][i]} vs {b['rec'][j]}"
    k = int(a["nk"][i])
    assert np.array_equal(bits(a["t"][:k, i]), bits(b["t"][:k, j])), f"{what}: knot epochs"
    assert np.array_equal(bits(a["y"][:k, :, i]), bits(b["y"][:k, :, j])), f"{what}: knot states"
    if events:
        assert [int(c[i]) for c in a["counts"]] == [int(c[j]) for c in b["counts"]], f"{what}: event counts / status"
        for x, y in zip(a["events"][i][0] + a["events"][i][1], b["events"][j][0] + b["events"][j][1]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: event lists"


def same_as_sources(out, srcs, source_of, craft_of, what, events=True):
    ro, rs = readable(out, events), [readable(s, events) for s in srcs]
    for i, (s, c) in enumerate(zip(source_of, craft_of)):
        same_craft(ro, i, rs[s], int(c), f"{what}: output craft {i} (craft {c} of source {s})", events)


def legs_and_gather(ea, method, parts, source_of, craft_of, make, what, after=None):
    """the pattern: sources of the scene craft `parts` to 0.4 T_END, gather (`make(sources)`), everything to T_END; the output against the
    oracle's single run of the craft each output craft came from and against the sources"""
    sc, res, lists = gather_preconditions(method)
    end = sc.calls[-1][1]
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    srcs = [batch_of(ea, eph, sc, method, p) for p in parts]
    for b in srcs:
        b.propagate(0.4 * end)
    before = [readable(b) for b in srcs]
    out = make(srcs)
    assert out.n == len(craft_of)
    same_as_sources(out, srcs, source_of, craft_of, f"{what}, at the gather")
    for s, b in enumerate(srcs):                           # the sources are not changed
        now = readable(b)
        for i in range(b.n):
            same_craft(now, i, before[s], i, f"{what}: source {s} after the gather")
    out.propagate(end)
    origin = [int(parts[s][c]) for s, c in zip(source_of, craft_of)]
    compare_sweep(out, [res[o] for o in origin], what)
    compare_events(out, [lists[o] for o in origin], what)
    for b in srcs:
        b.propagate(end)
    same_as_sources(out, srcs, source_of, craft_of, f"{what}, at the end")
    if after:
        after(out, srcs, source_of, craft_of)
    return out, srcs


def scrambled(n_from, n_take, seed, duplicates=2):
    """n_take craft of n_from in scrambled order, `duplicates` of them a second time"""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n_from)[:n_take - duplicates]
    idx = np.concatenate([idx, idx[:duplicates]])
    return idx[rng.permutation(len(idx))].astype(np.int64)


# ---- wave forms, in this process -------------------------------------------------------------------------------------------------------
def test_scrambled_select_with_duplicates(gpu):
    """1. a scrambled select of 40 craft of the 136, two of them twice (an FSAL pair: k[0] / k[S-1] travel)"""
    idx = scrambled(evs.T_N, 40, 1)
    assert len(set(idx.tolist())) == 38 and not np.array_equal(idx, np.sort(idx))
    legs_and_gather(gpu, FSAL_METHOD, [np.arange(evs.T_N)], [0] * 40, idx, lambda s: s[0].select(idx), "select 40")


def test_concat_of_three_batches(gpu):
    """2. concat of three batches of 50 / 1 / 85 craft"""
    parts = [np.arange(0, 50), np.arange(50, 51), np.arange(51, 136)]
    source_of = [0] * 50 + [1] + [2] * 85
    craft_of = list(range(50)) + [0] + list(range(85))
    legs_and_gather(gpu, METHOD, parts, source_of, craft_of, lambda s: gpu.SpacecraftBatch.concat(s), "concat 50 / 1 / 85")


def test_identity_gather_against_clone(gpu):
    """3. the identity gather is eph_craft_batch_clone: both continue alike"""
    clones = []

    def make(srcs):
        clones.append(srcs[0].clone())
        return gpu.SpacecraftBatch.gather(srcs, None, np.arange(evs.T_N))
    out, srcs = legs_and_gather(gpu, METHOD, [np.arange(evs.T_N)], [0] * evs.T_N, np.arange(evs.T_N), make, "identity")
    clones[0].propagate(SCENES[f"T-{METHOD}"].calls[-1][1])
    same_as_sources(out, clones, [0] * evs.T_N, np.arange(evs.T_N), "identity against clone")
    also = gpu.SpacecraftBatch.gather([clones[0]], [0] * evs.T_N, np.arange(evs.T_N))          # with an explicit source_of
    same_as_sources(also, clones, [0] * evs.T_N, np.arange(evs.T_N), "identity, explicit source_of")


def test_empty_output(gpu):
    """4. n_out == 0: an empty batch with the sources' configuration, on which every call works"""
    sc = SCENES[f"T-{METHOD}"]
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    src = batch_of(gpu, eph, sc, METHOD, np.arange(10))
    src.propagate(0.4 * sc.calls[-1][1])
    for out in (src.select([]), src.select(np.zeros(src.n, dtype=bool))):
        assert out.n == 0
        out.propagate(sc.calls[-1][1])
        assert len(out.summary()) == 0 and out.status()["status"].shape == (0,) and out.event_counts()[0].shape == (0,)
        out.reset_knots(), out.reset_events()
        assert out.clone().n == 0
        again = gpu.SpacecraftBatch.concat([out, src])                         # ... and it is a source like any other
        same_as_sources(again, [src], [0] * src.n, np.arange(src.n), "concat of an empty gather and its source")


def test_empty_source_among_the_sources(gpu):
    """5. a source batch of 0 craft among the sources"""
    parts = [np.arange(0, 70), np.arange(0, 0), np.arange(70, 136)]
    source_of = [0] * 70 + [2] * 66
    craft_of = list(range(70)) + list(range(66))
    legs_and_gather(gpu, METHOD, parts, source_of, craft_of, lambda s: gpu.SpacecraftBatch.concat(s), "concat 70 / 0 / 66")
    idx = scrambled(66, 30, 5)
    legs_and_gather(gpu, METHOD, parts, [2] * 30, idx, lambda s: gpu.SpacecraftBatch.gather(s, [2] * 30, idx), "gather from the third of three")


def test_event_search_position_travels(gpu):
    """the search position (ev_seg) is carried: after reset_events on both sides -- apsides dropped, the newest transition kept -- the
    output finds what its sources find and nothing a second time (a search that started over would find the dropped apsides again;
    without the reset it would only overwrite them with themselves)"""
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    parts = [np.arange(0, 60), np.arange(60, 136)]
    srcs = [batch_of(gpu, eph, sc, METHOD, p) for p in parts]
    for b in srcs:
        b.propagate(0.4 * end)
    dropped = sum(int(b.event_counts()[1].sum()) for b in srcs)
    assert dropped > 0
    idx = scrambled(60, 30, 3)
    source_of, craft_of = [0] * 30 + [1] * 76, idx.tolist() + list(range(76))
    out = gpu.SpacecraftBatch.gather(srcs, source_of, craft_of)
    for b in [out] + srcs:
        b.reset_events()
        b.propagate(end)
    same_as_sources(out, srcs, source_of, craft_of, "after reset_events")
    origin = [int(parts[s][c]) for s, c in zip(source_of, craft_of)]
    nap = out.event_counts()[1]
    assert sum(len(lists[o][1][0]) for o in origin) > int(nap.sum()) > 0                   # the dropped ones were not found again


# ---- thread forms: one child each ---------------------------------------------------------------------------------------------------
def slabs_and_eval_follow(out, srcs, source_of, craft_of):
    """eph_craft_batch_knot_slabs and eph_craft_batch_eval, the two readers that go through slot_of: the output's values are the
    sources' values for the same craft (the slabs: in same_as_sources; here the evaluation half way between every craft's knots 1, 2)"""
    ro = readable(out, False)
    at = np.stack([0.5 * (ro["t"][0] + ro["t"][1]), 0.25 * ro["t"][1] + 0.75 * ro["t"][2]])
    yo, io = out.eval(at, raw=True)
    assert io.all()
    for s, b in enumerate(srcs):
        mine = np.flatnonzero(np.asarray(source_of) == s)
        if len(mine) == 0:
            continue
        cs = np.asarray(craft_of)[mine]
        at_s = np.zeros((2, b.n))
        at_s[:, :] = readable(b, False)["t"][1][None, :]               # any epoch inside; overwritten for the craft that are asked
        at_s[:, cs] = at[:, mine]
        ys, ins = b.eval(at_s, raw=True)
        assert ins[:, cs].all()
        assert np.array_equal(bits(yo[:, :, mine]), bits(ys[:, :, cs])), f"eval of the output differs from source {s}'s"


def thread_form_cases(ea):
    n = evs.T_N
    rng = np.random.default_rng(7)
    # dealt -> dealt: 136 -> select of 130; dealt -> undealt: 136 -> select of 100
    for take in (130, 100):
        idx = scrambled(n, take, take)
        legs_and_gather(ea, METHOD, [np.arange(n)], [0] * take, idx, lambda s: s[0].select(idx), f"136 -> select of {take}", slabs_and_eval_follow)
    # undealt -> dealt: two batches of 68 (scrambled, one craft in both) -> concat of 136
    perm = rng.permutation(n)
    parts = [perm[:68].copy(), perm[68:].copy()]
    parts[1][5] = parts[0][9]
    out, srcs = legs_and_gather(ea, METHOD, parts, [0] * 68 + [1] * 68, list(range(68)) * 2, lambda s: ea.SpacecraftBatch.concat(s),
                                "two batches of 68 -> concat of 136", slabs_and_eval_follow)
    # undealt -> undealt: 68 -> select of 60
    idx = scrambled(68, 60, 60)
    legs_and_gather(ea, FSAL_METHOD, [parts[0]], [0] * 60, idx, lambda s: s[0].select(idx), "68 -> select of 60", slabs_and_eval_follow)


def run_child(argv, name, limit, **kwargs):
    """one child program on the device under its own timeout; after one that died of a signal or ran into its timeout no further
    child is started (the tests that would start one skip)"""
    if _dead_children:
        pytest.skip(f"the child of {_dead_children[0]} died: no further child is started")
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, capture_output=True, text=True, **kwargs)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _dead_children.append(name)
    return r


def run_case_child(case, env):
    r = run_child([sys.executable, str(ROOT / "tests" / "test_gpu_craft_gather.py"), case], case, 300, env=env, cwd=str(ROOT))
    assert r.returncode == 0 and f"{case} ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


@pytest.mark.parametrize("form", FORMS)
def test_gather_on_the_thread_forms(gpu, form):
    """the four combinations of dealt / undealt sides (source x output), each with the scramble and the duplicate, then knot_slabs and eval
    of the output against the sources'"""
    run_case_child(form, dict(os.environ, EPH_CRAFT_FORM="thread", EPH_CRAFT_QUEUE="1" if form == "thread-queue" else "0",
                              EPH_CRAFT_SORT="0" if form.endswith("undealt") else "2"))


# ---- FSAL registers and a pending retry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rearm_before", [False, True])
@pytest.mark.parametrize("method", [FSAL_METHOD, "Verner87"])
def test_failed_craft_resume_in_the_gathered_batch(gpu, pieces, method, rearm_before):
    """the craft fail at the table's end (EvalFailed: for an FSAL pair k[0] and k[S-1] are swapped and the failing stage zeroed); they
    are gathered, permuted, one craft twice; the table is appended; retry_failed (on the gathered batch, or on the source before the
    gather: the flag is carried) and propagate: bit-equal to the oracle's resumed run"""
    failed_craft_resume(gpu, pieces, method, rearm_before, [2, 0, 3, 1, 0], lambda batch, order: batch.select(order))


@pytest.mark.parametrize("rearm_before", [False, True])
def test_failed_craft_resume_in_a_clone(gpu, pieces, rearm_before):
    """the same through eph_craft_batch_clone, on the FSAL pair: klast, kfirst and the retry flag are read through a plain copy"""
    failed_craft_resume(gpu, pieces, FSAL_METHOD, rearm_before, [0, 1, 2, 3], lambda batch, order: batch.clone())


def failed_craft_resume(gpu, pieces, method, rearm_before, order, make):
    s, pcs = pieces
    ship = _ship()
    eph, olive = _live(gpu, s, pcs[0])
    n = 4
    pos, vel = _fleet(ship, n, 3)
    end = s.epoch + 6.5 * DAY
    batch = gpu.SpacecraftBatch(eph, ship.start, pos, vel, method, max_knots=8192)
    crafts = [orc.Craft(olive, s.mu, ship.start, pos[i], vel[i], method) for i in range(n)]
    batch.propagate(end)
    for i, c in enumerate(crafts):
        assert c.step_to(end) == orc.EVAL_FAILED
        _compare(batch, i, c, gpu.EVAL_FAILED, f"{method} craft {i}: the table's end")
    if rearm_before:
        batch.retry_failed()
    g = make(batch, order)
    for i, o in enumerate(order):
        _compare(g, i, crafts[o], gpu.EVAL_FAILED, f"{method} gathered craft {i}")
    both = [g, batch]                                     # the source is given the same calls, independently
    if not rearm_before:
        for b in both:
            b.propagate(end)                              # sticky in the gathered batch too
        for i, o in enumerate(order):
            _compare(g, i, crafts[o], gpu.EVAL_FAILED, f"{method} gathered craft {i}: sticky")
        for b in both:
            b.retry_failed()
    # a retry WITHOUT growth: one more failed attempt each. Its swap of k[0] and k[S-1] brings back what the gather carried as k[0]
    # (kfirst), which the retry after the growth then starts from
    for b in both:
        b.propagate(end)
    for c in crafts:
        assert c.step_to(end) == orc.EVAL_FAILED
    for i, o in enumerate(order):
        _compare(g, i, crafts[o], gpu.EVAL_FAILED, f"{method} gathered craft {i}: retried without growth")
    eph.append(pcs[1][0])
    assert olive.append(pcs[1][1])
    for b in both:
        b.retry_failed().propagate(end)
    for c in crafts:
        assert c.step_to(end) == 0
    for i, o in enumerate(order):
        _compare(g, i, crafts[o], 0, f"{method} gathered craft {i}: resumed")
    same_as_sources(g, [batch], [0] * len(order), order, f"{method}: gathered against the source", events=False)


def test_one_source_rearmed_and_one_not_is_refused(gpu, pieces):
    s, pcs = pieces
    ship = _ship()
    eph, _ = _live(gpu, s, pcs[0])
    pos, vel = _fleet(ship, 4, 3)
    a = gpu.SpacecraftBatch(eph, ship.start, pos[:2], vel[:2], FSAL_METHOD, max_knots=64)
    b = gpu.SpacecraftBatch(eph, ship.start, pos[2:], vel[2:], FSAL_METHOD, max_knots=64)
    a.retry_failed()
    st, out, text = raw_gather(gpu, [a, b], None, None)
    assert st == gpu.ERR_BAD_ARGUMENT and out is None and "retry_failed" in text and "source 1" in text, (st, out, text)
    with pytest.raises(ValueError, match="retry_failed"):
        gpu.SpacecraftBatch.concat([a, b])
    b.retry_failed()
    assert gpu.SpacecraftBatch.concat([a, b]).n == 4


# ---- timelines --------------------------------------------------------------------------------------------------------------------------
def _plans(sc, craft, mid):
    """burn lists of different lengths (0 .. 3), inertial and TNB about body 0; craft `mid` burns across 0.4 T_END"""
    end = sc.calls[-1][1]
    plans = []
    for q, i in enumerate(craft):
        burns = []
        for j in range(q % 4):
            t = end * (0.08 + 0.21 * j) + 37.0 * q
            burns.append((t, t + 400.0 + 50.0 * j, np.array([1e-4, -2e-4, 5e-5]) * (1 + j), -1 if (q + j) % 2 else 0))
        if i == mid:
            burns.append((0.4 * end - 1.0e4, 0.4 * end + 1.0e4, np.array([0.0, 1e-5, 0.0]), 0))
        plans.append(burns)
    return plans


def test_timelines_travel_and_restart(gpu):
    """sources with different burn counts per craft (inertial and TNB burns), gathered in the middle of a burn of one craft: propagate
    equals the oracle; eph_craft_batch_restart of the gathered batch with new plans gives the epochs, outcomes and subsequent knots that
    the restart of the sources gives (the host mirror of the CSR, t_start, cur_seg)"""
    sc = SCENES[f"T-{METHOD}"]
    end = sc.calls[-1][1]
    craft = np.arange(0, 22, 2)                                       # 11 craft
    mid = int(craft[np.argmin(sc.a[craft])])                          # the shortest orbit: the smallest steps
    plans = dict(zip(craft.tolist(), _plans(sc, craft, mid)))
    assert len({len(p) for p in plans.values()}) >= 4
    burns = [plans.get(i, []) for i in range(sc.n)]
    sol = orc.Solution.from_parts(*sc.table)
    p = sc.params
    oracle = {}
    for i in craft:
        c = orc.Craft(sol, sc.mu, sc.t0[i], sc.pos[i], sc.vel[i], METHOD, h_init=p["h_init"], h_max=p["h_max"], tol_pos=p["tol_pos"],
                      tol_vel=p["tol_vel"], burns=burns[i], soi_radius=sc.soi)
        assert c.step_to(0.4 * end) == 0
        if i == mid:
            t = c.state()["t"]
            assert 0.4 * end - 1.0e4 < t < 0.4 * end + 1.0e4, "the gather is not taken inside the burn"
        oracle[int(i)] = c
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    parts = [craft[:6], craft[6:]]
    srcs = [batch_of(gpu, eph, sc, METHOD, q, burns=burns, max_knots=2000) for q in parts]
    for b in srcs:
        b.propagate(0.4 * end)
    source_of = [1, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    craft_of = [4, 5, 0, 0, 3, 2, 1, 3, 2, 1, 4, 4]                  # every craft, scrambled; craft 4 of source 1 twice
    out = gpu.SpacecraftBatch.gather(srcs, source_of, craft_of)
    origin = [int(parts[s][c]) for s, c in zip(source_of, craft_of)]
    assert mid in origin and sorted(set(origin)) == craft.tolist()
    same_as_sources(out, srcs, source_of, craft_of, "timelines, at the gather")
    out.propagate(end)
    for o in sorted(set(origin)):
        assert oracle[o].step_to(end) == 0
    res = [dict(status=0, craft=oracle[o]) for o in origin]
    compare_sweep(out, res, "timelines")
    compare_events(out, [(r["craft"].transitions(), r["craft"].apsides()) for r in res], "timelines")
    for b in srcs:
        b.propagate(end)
    # new plans: the last burn 1 % stronger, or a burn added late, or the plan unchanged
    def edited(i, k):
        b = list(burns[i])
        if k % 3 == 0 and b:
            s0, e0, a0, r0 = b[-1]
            b[-1] = (s0, e0, np.asarray(a0) * 1.01, r0)
        elif k % 3 == 1:
            b.append((0.7 * end, 0.7 * end + 300.0, np.array([1e-4, 0.0, 0.0]), -1))
        return b
    new = {int(i): edited(int(i), k) for k, i in enumerate(craft)}
    eo, oo = out.restart([new[o] for o in origin])
    later = 1.2 * end
    out.propagate(later)
    for s, b in enumerate(srcs):
        es, os_ = b.restart([new[int(i)] for i in parts[s]])
        b.propagate(later)
        mine = [i for i, q in enumerate(source_of) if q == s]
        cs = [craft_of[i] for i in mine]
        assert same(eo[mine], es[cs]) and np.array_equal(oo[mine], os_[cs]), f"restart epochs / outcomes of source {s}"
    assert len(set(eo.tolist())) >= 2 and (oo == 0).any()
    same_as_sources(out, srcs, source_of, craft_of, "timelines, after the restart")


# ---- depths ----------------------------------------------------------------------------------------------------------------------------
def test_a_full_knot_slab_continues_in_a_deeper_batch(gpu):
    """a source of max_knots = 40 holding EPH_KNOTS_FULL craft, gathered with a source of depth 400: the full craft continue without a
    drain and equal the oracle's undrained run"""
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    nk = np.array([len(r["craft"].knots()[0]) for r in res])
    shallow = np.concatenate([np.flatnonzero(nk > 60)[:6], np.flatnonzero(nk <= 40)[:3]])
    deep = np.setdiff1d(np.arange(sc.n), shallow)[:20]
    assert (nk[shallow] > 60).sum() >= 3 and (nk[shallow] <= 40).sum() >= 1
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    a = batch_of(gpu, eph, sc, METHOD, shallow, max_knots=40)
    b = batch_of(gpu, eph, sc, METHOD, deep)
    a.propagate(end)
    b.propagate(0.4 * end)
    st = a.status()
    assert ((st["status"] == KNOTS_FULL) == (nk[shallow] > 40)).all() and (st["nknots"][st["status"] == KNOTS_FULL] == 40).all()
    out = gpu.SpacecraftBatch.concat([a, b])
    source_of, craft_of = [0] * len(shallow) + [1] * len(deep), list(range(len(shallow))) + list(range(len(deep)))
    same_as_sources(out, [a, b], source_of, craft_of, "depths, at the gather")          # (the status still reads KNOTS_FULL)
    out.propagate(end)
    origin = np.concatenate([shallow, deep])
    compare_sweep(out, [res[o] for o in origin], "depths")
    compare_events(out, [lists[o] for o in origin], "depths")
    t, y = out.knot_slabs(0, 400)                                                       # the output's depth is the deeper one
    assert t.shape == (400, out.n)


def test_a_full_event_slab_stays_full_until_reset(gpu):
    """an EPH_EVENTS_FULL craft (scene F-ap, slabs of 3) gathered with a source of deeper event slabs stays full until reset_events; the
    lists read before and after the reset, merged as a caller holding the reference's types would, equal the oracle's"""
    sc = DRAINED["F-ap"]
    method = sc.methods[0]
    res, lists = oracle_results("F-ap", method)
    end = sc.calls[-1][1]
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    a = batch_of(gpu, eph, sc, method, np.arange(sc.n))                                  # max_tr = max_ap = 3
    b = batch_of(gpu, eph, sc, method, np.arange(sc.n), max_tr=16, max_ap=64)
    a.propagate(end)
    b.propagate(0.3 * end)
    assert (a.event_counts()[2] == evs.EVENTS_FULL).all()
    out = gpu.SpacecraftBatch.concat([a, b])
    n = sc.n
    same_as_sources(out, [a, b], [0] * n + [1] * n, list(range(n)) * 2, "event depths, at the gather")
    first = out.event_counts()
    out.propagate(end)
    counts = out.event_counts()
    assert (counts[2][:n] == evs.EVENTS_FULL).all() and (counts[2][n:] == 0).all()
    assert np.array_equal(counts[0][:n], first[0][:n]) and np.array_equal(counts[1][:n], first[1][:n])      # sticky: nothing was searched
    tr_reads, ap_reads = [[] for _ in range(2 * n)], [[] for _ in range(2 * n)]

    def read():
        c = out.event_counts()
        for i in range(2 * n):
            (tt, tb), (at, ad, ab, ak) = out.events(i, c)
            tr_reads[i].append(list(zip(tt.tolist(), tb.tolist())))
            ap_reads[i].append(list(zip(at.tolist(), ad.tolist(), ab.tolist(), ak.tolist())))
        return c
    read()
    out.reset_events()
    out.propagate(end)
    c = read()
    assert not c[2].any(), c[2]                                                          # 16 / 64 entries are room enough
    compare_sweep(out, res + res, "event depths")
    for i in range(2 * n):
        (ott, otb), (oat, oad, oab, oak) = lists[i % n]
        mt, ma = evs.merge_transitions(tr_reads[i]), evs.merge_apsides(ap_reads[i])
        assert same([x[0] for x in mt], ott) and [x[1] for x in mt] == otb.tolist(), f"craft {i}: merged transitions {mt}"
        assert same([x[0] for x in ma], oat) and same([x[1] for x in ma], oad), f"craft {i}: merged apsides {ma}"
        assert [x[2] for x in ma] == oab.tolist() and [x[3] for x in ma] == oak.tolist(), f"craft {i}: merged apsides {ma}"


# ---- disagreements ------------------------------------------------------------------------------------------------------------------
def test_sources_that_disagree_are_refused(gpu):
    """one refusal each for another ephemeris, method, parameter byte, body order, events on / off and SOI radius: *out is NULL, the
    text names the disagreement, and the sources' summaries are unchanged"""
    sc = SCENES[f"T-{METHOD}"]
    eph = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    eph2 = gpu.Ephemeris(gpu.Solution.from_parts(*sc.table), sc.mu)
    idx = np.arange(6)
    a = batch_of(gpu, eph, sc, METHOD, idx)
    a.propagate(0.1 * sc.calls[-1][1])
    p2 = params_of(gpu, sc)
    p2.tol_velocity = float(np.nextafter(p2.tol_velocity, 1.0))
    soi2 = sc.soi.copy()
    soi2[3] = np.nextafter(soi2[3], 0.0)
    order = np.arange(sc.n_bodies, dtype=np.int32)
    order[[1, 2]] = order[[2, 1]]
    others = {"ephemeris": batch_of(gpu, eph2, sc, METHOD, idx),
              "method": batch_of(gpu, eph, sc, FSAL_METHOD, idx),
              "adaptive parameters": batch_of(gpu, eph, sc, METHOD, idx, params=p2),
              "body order": batch_of(gpu, eph, sc, METHOD, idx).set_body_order(order),
              "events on / off": batch_of(gpu, eph, sc, METHOD, idx, events=False),
              "soi radii": batch_of(gpu, eph, sc, METHOD, idx, soi=soi2)}
    for what, b in others.items():
        before = a.summary().tobytes(), b.summary().tobytes()
        st, out, text = raw_gather(gpu, [a, b], [1, 0, 1], [0, 5, 2])
        assert st == gpu.ERR_BAD_ARGUMENT and out is None and what in text and "source 1" in text, (what, st, out, text)
        with pytest.raises(ValueError, match=what):
            gpu.SpacecraftBatch.concat([a, b])
        assert (a.summary().tobytes(), b.summary().tobytes()) == before, what
    # the index and argument rules, where a handle exists
    for so, co, n_out, what in (([0, 2], [0, 0], None, "source_of[1]"), ([0, 1], [0, 6], None, "craft_of[1]"), ([0, 1], [-1, 0], None, "craft_of[0]"),
                                (None, None, 11, "sum of the sources' sizes"), (None, [0, 1], None, "n_sources == 1"), ([0, 1], None, 2, "source_of == NULL")):
        st, out, text = raw_gather(gpu, [a, a], so, co, n_out)
        assert st == gpu.ERR_BAD_ARGUMENT and out is None and what in text, (what, st, out, text)
    st, out, text = raw_gather(gpu, [a], None, [0], -1)
    assert st == gpu.ERR_BAD_ARGUMENT and out is None and "n_out < 0" in text
    assert gpu.SpacecraftBatch.concat([a, a]).n == 12                                    # the same batch twice is fine


# ---- commit rule ---------------------------------------------------------------------------------------------------------------------
# Device allocations each call makes for the batch its case builds: the number of k at which the call fails before it first succeeds.
# Every buffer of the batch is one of them, so a buffer dropped from (or added to) a call moves its count.
ALLOCATIONS = {"commit-rule": 35,      # gather (no body order set): 20 of the state, the index scratch, 10 event slabs, soi, 3 of the deal
               "clone-rule": 34,       # every buffer of the source but `summary`: 33 copied, the queue fresh
               "create-rule": 23,      # 20 of the state, 3 of the deal
               "events-rule": 11}      # soi, 4 per-craft event arrays, 6 event slabs


def unchanged(batches, before, what):
    for s, b in enumerate(batches):
        now = readable(b)
        for i in range(b.n):
            same_craft(now, i, before[s], i, f"{what}: source {s}")


def commit_rule_case(ea):
    """fail the k-th allocation for every k the call makes: an error status, *out NULL, the sources bit-equal to a snapshot; then the call
    succeeds and is correct. Thread form: the deal's own allocations are among them"""
    import hooks
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    parts = [np.arange(0, 100), np.arange(100, 136)]
    srcs = [batch_of(ea, eph, sc, METHOD, p) for p in parts]
    for b in srcs:
        b.propagate(0.4 * end)
    rng = np.random.default_rng(11)
    source_of = rng.integers(0, 2, 132).astype(np.int32)
    craft_of = np.where(source_of == 0, rng.integers(0, 100, 132), rng.integers(0, 36, 132)).astype(np.int64)
    before = [readable(b) for b in srcs]

    def failed(k, out):
        assert out is None, (k, out)
        unchanged(srcs, before, f"k = {k}")
    failures, out = failing_allocations(ea, hooks.load(), lambda: raw_gather(ea, srcs, source_of, craft_of), failed)
    assert failures >= 30, failures                                      # every per-craft array, the slabs, the event slabs, the deal
    good = ea.SpacecraftBatch._adopt(C.c_void_p(out), ephemeris=eph, n=len(craft_of), params=srcs[0].params)
    same_as_sources(good, srcs, source_of, craft_of, "after the failures, at the gather")
    good.propagate(end)
    origin = [int(parts[s][c]) for s, c in zip(source_of, craft_of)]
    compare_sweep(good, [res[o] for o in origin], "after the failures")
    compare_events(good, [lists[o] for o in origin], "after the failures")
    return failures


def swapped_order(sc):
    """a non-identity body order. Only body 0 of scene T has mass, so the sums keep their bits and the oracle's run stays the reference"""
    order = np.arange(sc.n_bodies, dtype=np.int32)
    order[[1, 2]] = order[[2, 1]]
    return order


def full_batch(ea, eph, sc):
    """the 136 craft as a batch that owns every optional buffer: dealt (thread form), events on, a body order set"""
    return batch_of(ea, eph, sc, METHOD, np.arange(sc.n)).set_body_order(swapped_order(sc))


def attributes_of(b):
    return {k: v for k, v in vars(b).items() if k not in ("_L", "_h", "_owned")}


def clone_rule_case(ea):
    """eph_craft_batch_clone under the same rule: every failure leaves *out NULL and the source as it was; the first success is the source,
    and goes on like it and like the oracle"""
    import hooks
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    src = full_batch(ea, eph, sc)
    src.propagate(0.4 * end)
    before = [readable(src)]

    def raw_clone():
        out = C.c_void_p(0x5A5A5A5A)
        st = ea._lib().eph_craft_batch_clone(src._h, C.byref(out))
        return st, out.value, ea._lib().eph_last_error().decode()

    def failed(k, out):
        assert out is None, (k, out)
        unchanged([src], before, f"k = {k}")
    failures, out = failing_allocations(ea, hooks.load(), raw_clone, failed)
    good = ea.SpacecraftBatch._adopt(C.c_void_p(out), **attributes_of(src))
    everyone = [0] * sc.n, np.arange(sc.n)
    same_as_sources(good, [src], *everyone, "after the failures, at the clone")
    for b in (good, src):
        b.propagate(end)
    same_as_sources(good, [src], *everyone, "after the failures, at the end")
    compare_sweep(good, res, "clone after the failures")
    compare_events(good, lists, "clone after the failures")
    return failures


def create_rule_case(ea):
    """eph_craft_batch_create under the same rule: `out` is written on success only; the first success, its events enabled, runs like the
    oracle and like a batch created with no failure injected"""
    import hooks
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    params = params_of(ea, sc)
    t0, pos, vel = ea._f64(sc.t0), ea._f64(sc.pos).reshape(-1, 3), ea._f64(sc.vel).reshape(-1, 3)
    untouched = 0x5A5A5A5A

    def raw_create():
        out = C.c_void_p(untouched)
        st = ea._lib().eph_craft_batch_create(eph._h, sc.n, ea._p(t0), ea._p(pos), ea._p(vel), METHOD.encode(), C.byref(params),
                                              *ea._burn_csr(sc.burns, sc.n), int(sc.max_knots), C.byref(out))
        return st, out.value, ea._lib().eph_last_error().decode()

    def failed(k, out):
        assert out == untouched, (k, out)
    failures, out = failing_allocations(ea, hooks.load(), raw_create, failed)
    good = ea.SpacecraftBatch._adopt(C.c_void_p(out), ephemeris=eph, n=sc.n, params=params)
    plain = batch_of(ea, eph, sc, METHOD, np.arange(sc.n), events=False)
    for b in (good, plain):
        b.enable_events(sc.soi, max_transitions=sc.max_tr, max_apsides=sc.max_ap).set_body_order(swapped_order(sc))
        b.propagate(end)
    same_as_sources(good, [plain], [0] * sc.n, np.arange(sc.n), "created after the failures against a plain creation")
    compare_sweep(good, res, "created after the failures")
    compare_events(good, lists, "created after the failures")
    return failures


def events_rule_case(ea):
    """eph_craft_batch_enable_events failing at its k-th allocation leaves a batch on which a second call succeeds, and which then runs
    bit for bit like a batch whose first call succeeded (and like the oracle)"""
    import hooks
    H = hooks.load()
    sc, res, lists = gather_preconditions(METHOD)
    end = sc.calls[-1][1]
    eph = ea.Ephemeris(ea.Solution.from_parts(*sc.table), sc.mu)
    soi = ea._f64(sc.soi)
    reference = full_batch(ea, eph, sc)
    reference.propagate(end)
    compare_sweep(reference, res, "enabled at once")
    compare_events(reference, lists, "enabled at once")
    want = readable(reference)
    for k in range(1, 200):
        b = batch_of(ea, eph, sc, METHOD, np.arange(sc.n), events=False).set_body_order(swapped_order(sc))
        assert H.fail_alloc(k) == 0
        st = ea._lib().eph_craft_batch_enable_events(b._h, ea._p(soi), int(sc.max_tr), int(sc.max_ap))
        text, left = ea._lib().eph_last_error().decode(), H.fail_alloc(0)
        if st == ea.OK:
            return k - 1
        assert st == ea.ERR_OUT_OF_MEMORY and "injected allocation failure" in text and left == 0, (k, st, text, left)
        b.enable_events(sc.soi, max_transitions=sc.max_tr, max_apsides=sc.max_ap)
        b.propagate(end)
        got = readable(b)
        for i in range(b.n):
            same_craft(got, i, want, i, f"enabled at the second call after a failure at allocation {k}: craft {i}")
    raise AssertionError("no success by k = 199")


RULE_CASES = {"commit-rule": commit_rule_case, "clone-rule": clone_rule_case, "create-rule": create_rule_case, "events-rule": events_rule_case}


def run_rule_child(case):
    run_case_child(case, dict(os.environ, EPH_AMD_LIBRARY=str(HOOKS_LIB), EPH_CRAFT_FORM="thread", EPH_CRAFT_SORT="2", EPH_CRAFT_QUEUE="0"))


def test_commit_rule_under_failing_allocations(gpu):
    run_rule_child("commit-rule")


@pytest.mark.parametrize("case", ["clone-rule", "create-rule", "events-rule"])
def test_lifecycle_calls_under_failing_allocations(gpu, case):
    """create, clone and enable_events of the 136-craft batch that owns every optional buffer, each in a child like the gather's"""
    run_rule_child(case)


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_cpp_example_fleet_digests_agree(gpu, tmp_path):
    """examples/craft_fleet.cpp builds against the library alone, runs once, and every ship of the fleet has the digest of the same ship
    flown alone"""
    exe = tmp_path / "craft_fleet"
    libdir = ROOT / "ephemeris_explorer_amd"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT / 'include'}", str(ROOT / "examples" / "craft_fleet.cpp"), f"-L{libdir}",
                           "-lephemeris_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = run_child([str(exe)], "craft_fleet", 120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("ship-")]
    assert [l.split()[0] for l in lines] == ["ship-2", "ship-3", "ship-4"] and "MISMATCH" not in r.stdout, r.stdout


# ---- the children ----------------------------------------------------------------------------------------------------------------------
if __name__ == "__main__":
    import ephemeris_explorer_amd as ea
    case = sys.argv[1]
    try:
        if case in RULE_CASES:
            failures = RULE_CASES[case](ea)
            print(f"{case}: failures {failures}")
            assert failures == ALLOCATIONS[case], f"{failures} allocations, {ALLOCATIONS[case]} before"
        else:
            assert os.environ.get("EPH_CRAFT_FORM") == "thread"
            thread_form_cases(ea)
    except AssertionError as e:
        print(f"{case} FAILED: {str(e)[:1500]}")
        raise
    print(f"{case} ok")
