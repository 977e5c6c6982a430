"""CPU: the scenarios of tests/wg_solout_scenes.py on the C oracle alone. Conditions, not measurements: each scenario still steps on what it
was planted for (tests/test_gpu_wg_solout.py compares the device with these very runs, so a scenario that went quiet would check
nothing), and the C oracle is pinned to the Python restatement on the 130-body scenario (the restatement's all-pairs sum is pure
Python: ~0.03 s per evaluation at 130 bodies, minutes at 705)."""
import numpy as np
import pytest

import wg_solout_scenes as ws
from oracle import orc
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def records():
    return {sc.name: ws.run_oracle(sc) for sc in ws.SCENES}


def _steps(rec, handle=0):
    """step count after every operation of one handle: {operation index: steps}"""
    t = rec["times"]
    return {int(r[0]): int(r[4]) for r in t if int(r[1]) == handle}


def _takes(sc):
    return [k for k, op in enumerate(sc.ops) if op[0] == "take"]


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
def test_sizes_and_partly_empty_last_workgroups(sc):
    """what the sizes are there for, from the numbers alone"""
    assert sc.n in (130, 330, 705) and (sc.n + 63) // 64 in (3, 6, 12)
    if sc.n == 705:
        assert [sc.n % wb for wb in (16, 8, 4)] == [1, 1, 1]
    if sc.n == 330:
        assert [sc.n % wb for wb in (16, 8, 4)] == [10, 2, 2]
    assert len(set(sc.count[:5].tolist())) >= 4 and len(set(sc.degree[:6].tolist())) >= 5       # neighbouring lanes differ
    assert {s.method for s in ws.SCENES} == {"QuinlanTremaine12", "Stormer13"} and {s.direction for s in ws.SCENES} == {1, -1}


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
def test_the_operations_do_what_the_list_says(sc, records):
    """step counts follow the list (so the conditions below may be computed from it), both handles end alike, step_to went past its time"""
    rec, steps, done = records[sc.name], _steps(records[sc.name]), 0
    for k, op in enumerate(sc.ops):
        if op[0] == "step":
            done += 1
        elif op[0] == "step_n":
            done += op[1]
        elif op[0] == "step_to":
            assert steps[k] >= done + int(np.ceil(op[1])), (sc.name, k, steps[k], done)
            done = steps[k]
        assert steps[k] == done, (sc.name, k, op, steps[k], done)
    assert _steps(rec, 1)[len(sc.ops) - 1] == done                                   # the clone went the same way
    assert done > sc.startup() + 100                                                # most of the run is the fused kernel's
    for key in ("pos", "vel", "t"):
        assert np.array_equal(ws.bits(rec[f"final0_{key}"]), ws.bits(rec[f"final1_{key}"]))
    last = _takes(sc)[-1]
    for what in ("info", "npoly", "ncoef", "coef"):
        assert np.array_equal(ws.bits(rec[f"take{last}_0_{what}"]), ws.bits(rec[f"take{last}_1_{what}"]))


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
def test_every_sampling_body_has_two_polynomials(sc, records):
    """by the last take every body with a nonzero period has handed over at least 2 polynomials (all takes of the original together),
    and exactly as many as its period says"""
    rec, m = records[sc.name], sc.periods()
    total = sum(rec[f"take{k}_0_npoly"] for k in _takes(sc))
    done = _steps(rec)[len(sc.ops) - 1]
    assert (total[m > 0] >= 2).all(), (sc.name, np.flatnonzero((m > 0) & (total < 2))[:5])
    assert np.array_equal(total, np.where(m > 0, done // np.maximum(m, 1) // ws.KDIV, 0))
    assert (total[m == 0] == 0).all()
    assert rec[f"take{_takes(sc)[-1]}_0_ncoef"].min() >= 3 and len(set(rec[f"take{_takes(sc)[-1]}_0_ncoef"].tolist())) >= 5      # degree + 1 rows


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
def test_a_take_with_partly_filled_windows(sc, records):
    """at least one take happens while some body holds a partly filled window (samples taken, the ninth not yet): the solution that
    begins there starts BEFORE the integrator's time, by what the window holds"""
    rec, m, steps = records[sc.name], sc.periods(), _steps(records[sc.name])
    takes = _takes(sc)
    partly = {k: (m > 0) & ((steps[k] // np.maximum(m, 1)) % ws.KDIV != 0) for k in takes}
    assert any(p.any() for p in partly.values()), sc.name
    first, second = takes[0], takes[-1]
    assert partly[first].sum() * 2 >= (m > 0).sum(), (sc.name, int(partly[first].sum()))          # and not a lone body: half of them
    t_first = rec["times"][(rec["times"][:, 0] == first) & (rec["times"][:, 1] == 0)][0, 3]
    start = rec[f"take{second}_0_info"][:, 0]
    if sc.direction < 0:                               # push_front moved the start by one interval per polynomial since
        start = start + rec[f"take{second}_0_info"][:, 1] * rec[f"take{second}_0_npoly"]
    before = (t_first - start) * sc.direction > 0.5 * sc.dt
    assert (before[partly[first]]).all(), sc.name


@pytest.mark.parametrize("sc", ws.SCENES, ids=lambda s: s.name)
def test_batches_begin_in_mid_period(sc, records):
    """at least three batches begin with a nonzero phase (steps since the body's last sample) for at least half of the bodies that
    sample at all: phase = steps done mod period, period by trigger_period's rule (`count` when dt * count accumulates exactly, else
    0: such a body has no phase). Past the start-up at least two of them: those are the fused kernel's batches."""
    m, steps = sc.periods(), _steps(records[sc.name])
    live = m > 0
    assert np.array_equal(m[live], sc.count[live].astype(np.int64))
    # where batches begin (propagator.cpp: step_n runs the start-up one step per batch, the rest of a call in one; single steps past
    # the start-up queue up and run as one batch; step_to's later batches are not counted)
    before = [0] + [steps[k] for k in range(len(sc.ops) - 1)]
    starts, queued = [], False
    for k, op in enumerate(sc.ops):
        if op[0] not in ("step", "step_n", "step_to"):
            queued = False
            continue
        starts += range(before[k], min(steps[k], sc.startup()))
        if steps[k] > sc.startup() and not (queued and op[0] == "step"):
            starts.append(max(before[k], sc.startup()))
        queued = op[0] == "step" and before[k] >= sc.startup()
    mid = [s for s in starts if ((s % np.maximum(m, 1))[live] != 0).sum() * 2 >= live.sum()]
    assert len(mid) >= 3 and any(s >= sc.startup() for s in mid), (sc.name, starts, mid)
    # and of the fused kernel's batches (past the start-up), every period above 1 begins at least one in mid-period, with a carried
    # window (samples in the log region from earlier batches) at least once
    steady = [s for s in starts if s >= sc.startup()]
    assert len(steady) >= 4, (sc.name, steady)
    for period in sorted(set(m[m > 1].tolist())):
        assert any(s % period for s in steady), (sc.name, period, steady)
        assert any((s // period) % ws.KDIV for s in steady), (sc.name, period, steady)


def test_the_step_that_is_not_representable(records):
    """dt = 0.7: bodies that never sample (period 0) between bodies that do, in every wave, after the first window and at the end"""
    sc = ws.by_name("p330-m0")
    rec, m = records[sc.name], sc.periods()
    assert set(m.tolist()) == {0, 1, 3} and m[1] == 0 and m[0] == 3 and m[2] == 1             # 0.7 * 10 and 0.7 * 7 are stepped over
    first = rec[f"take{_takes(sc)[0]}_0_npoly"]
    assert _steps(rec)[_takes(sc)[0]] >= 3 * ws.KDIV                                          # count 3's first window is over
    assert (first[m == 0] == 0).all() and (first[m > 0] > 0).all() and (m == 0).any() and (m > 0).any()
    quad = (m.reshape(-1, 2)[:, 0] > 0) & (m.reshape(-1, 2)[:, 1] == 0)                       # neighbours: live, dead, live, dead
    assert quad.all()
    # the never-sampled bodies hold time() at the start (to the rounding of `t - last_sample_time` after a take: the accumulated
    # sum is not the integrator's time, and those bits are compared too): the system has reached nothing
    assert (np.abs(rec["times"][:, 2]) < 1e-12).all() and (rec["times"][:, 2] != 0.0).any()


def test_the_partition_scenario_ends_its_batches_on_fitted_samples():
    """SHARD: the sharded batches' last steps are the only launches without do_predict (nbody.cpp: `s < k || leave_prediction`, and a
    sharded handle leaves no prediction behind). Each of those steps stores samples, one of the batches has a single step, and the
    take has fitted every one of those samples: a store skipped or misplaced there shows in a polynomial"""
    sc = ws.SHARD
    rec, m = ws.run_oracle(sc), sc.periods()
    steps = _steps(rec)
    ends = [steps[k] for k, op in enumerate(sc.ops) if op[0] == "step_n"][1:]           # the first call runs before the partition
    assert steps[0] == sc.startup() and len(ends) == 3 and 1 in np.diff([steps[0]] + ends)
    npoly = rec[f"take{len(sc.ops) - 1}_0_npoly"]
    for end in ends:
        stored = (m > 0) & (end % np.maximum(m, 1) == 0)                                 # bodies that sample on that step
        fitted = stored & (end // np.maximum(m, 1) <= ws.KDIV * npoly)
        assert fitted.sum() >= sc.n // 5, (end, int(stored.sum()), int(fitted.sum()))
        assert fitted[:384].any() and fitted[384:].any()                                 # on both ranks
    assert npoly[sc.n - 1] > 0                                                           # the body alone in the last workgroup


def test_c_oracle_against_the_python_restatement(records):
    """orc.Propagator (what the device is compared with) against pyoracle.Propagator on the 130-body scenario: the original handle's
    steps (the restatement has no step_to and no clone: it is stepped as often as the C oracle stepped), every take, the final state"""
    sc = ws.by_name("p130")
    rec, steps = records[sc.name], _steps(records[sc.name])
    pos, vel, mu = sc.system()
    p = po.Propagator(pos, vel, mu, 0.0, sc.dt, sc.direction, sc.count, sc.degree, sc.method)
    done = 0
    for k, op in enumerate(sc.ops):
        while done < steps[k]:
            assert p.step() == 0
            done += 1
        if op[0] != "take":
            continue
        sol = p.take_solution()
        info, npoly, nc, co = (rec[f"take{k}_0_{w}"] for w in ("info", "npoly", "ncoef", "coef"))
        q = 0
        for b in range(sc.n):
            assert (sol[b]["start"], sol[b]["interval"], len(sol[b]["polys"])) == (info[b, 0], info[b, 1], npoly[b]), (k, b)
            for poly in sol[b]["polys"]:
                assert nc[q] == len(poly), (k, b)
                want = np.zeros((8, 3))
                want[:len(poly)] = [[float(x) for x in v] for v in poly]
                assert np.array_equal(ws.bits(co[q]), ws.bits(want)), (k, b, q)
                q += 1
        assert q == len(nc)
    assert p.p.time == rec["final0_t"][0]
    assert np.array_equal(ws.bits(np.array([[float(c) for c in r] for r in p.p.y])), ws.bits(rec["final0_pos"]))
    assert np.array_equal(ws.bits(np.array([[float(c) for c in r] for r in p.p.dy])), ws.bits(rec["final0_vel"]))


def test_compare_names_operation_and_body(records):
    """the comparison the GPU children use: equal runs pass, one flipped bit in one coefficient is found and named"""
    sc = ws.by_name("p130")
    rec = records[sc.name]
    ws.compare(dict(rec), rec, "self", sc)
    last = _takes(sc)[-1]
    bad = dict(rec)
    co = rec[f"take{last}_0_coef"].copy()
    q = int(np.cumsum(rec[f"take{last}_0_npoly"])[128])              # body 129's first polynomial
    co[q, 1, 2] = np.nextafter(co[q, 1, 2], np.inf)
    bad[f"take{last}_0_coef"] = co
    with pytest.raises(AssertionError, match=rf"p130: op {last} .*body 129 "):
        ws.compare(bad, rec, "flipped", sc)
    bad = dict(rec)
    tm = rec["times"].copy()
    tm[4, 3] = np.nextafter(tm[4, 3], np.inf)
    bad["times"] = tm
    with pytest.raises(AssertionError, match=r"p130: op 4 \('step_n', 20\) handle 0"):
        ws.compare(bad, rec, "flipped", sc)
    assert ws.targets_of(rec) == [float(rec["times"][rec["times"][:, 0] == 9][0, 5])]
