"""Scenarios for the solout sample that k_lm_step_wg's tail wave stores (csrc/step_wg.hip: `maybe_sample(a.samp, my_i, cc, a.step, yv[0])`
behind the force, the Cowell velocity and in front of the predictor), shared by tests/test_wg_solout_scenes.py (CPU: the C oracle alone,
and against the Python restatement) and tests/test_gpu_wg_solout.py (every workgroup form against the C oracle). A plain module, no
fixtures.

A scenario is a pure description -- n bodies of workloads.plummer, method, direction, dt, the cycles that give every body its `count`
and `degree`, and a fixed list of operations -- and `run()` plays it on anything with the propagator's methods: orc.Propagator,
ephemeris_explorer_amd.NBodyPropagator. What is planted, and for what:

  sizes     130, 330, 705: 3, 6 and 12 source tiles. 705 = 44 * 16 + 1 = 88 * 8 + 1 = 176 * 4 + 1: the last workgroup of every form owns
            ONE body; 330 leaves it 10 of 16, 2 of 8, 2 of 4 (the `my_i < a.hi` half of `owner`).
  counts    [1, 2, 3, 7, 12] by body index (degrees 2 .. 7): neighbouring lanes of one tail wave sample at different steps into log
            regions at different fill levels, so a sample of the wrong level, step, body or component lands in some body's window.
  OPS       chunk lengths that share no factor with the periods: batches begin with nonzero `phase` and a carried window. Three single
            step() calls (inside the start-up they run at once; the deferred queue is OPS_M0's), step_n(5) inside the start-up (k_sample,
            not the fused store), step_n(20) across its end (the first fused batch, the one that begins with k_lm_predict), a take,
            step_n(1) (a batch of one step), step_n(61), a clone, step_to 37.5 steps ahead on both, takes on both. (A handle of more
            than 64 bodies that is not sharded leaves the next level's prediction behind, nbody.cpp: every step of these batches has
            do_predict set. The arm without it is SHARD's.)
  Stormer13 L = 13 (the other instantiation of every form); BACKWARD: negative h, windows fitted back to front, push_front.
  m0        dt = 0.7, counts [3, 10, 1, 7]: 0.7 * 10 is stepped over by the accumulated sum (nbody.rs:389-391), those bodies' period is 0
            and they sit between live lanes of one wave (the `m == 0` arm of maybe_sample). Such a system never reaches any time, so
            its list has step_n where OPS has step_to, and single steps once more after the start-up (the deferred queue).

`DISPATCH` are the sizes that reach the workgroup forms with nothing forced (dispatch.cpp: 4 bodies per workgroup up to 1024 targets,
the six-wave form up to 2048, 16 above)."""
import numpy as np

H = 1.0 / 1024.0
FORWARD, BACKWARD = 1, -1
KDIV = 8                                           # samples per window (sharing end points): one polynomial per 8 periods

OPS = (("step",), ("step",), ("step",), ("step_n", 5), ("step_n", 20), ("take",), ("step_n", 1), ("step_n", 61), ("clone",),
       ("step_to", 37.5), ("take",))
OPS_M0 = (("step",), ("step",), ("step",), ("step_n", 5), ("step_n", 20), ("take",), ("step_n", 1), ("step",), ("step",), ("step_n", 59),
          ("clone",), ("step_n", 38), ("take",))


class Scenario:
    def __init__(self, name, n, method="QuinlanTremaine12", direction=FORWARD, dt=H, counts=(1, 2, 3, 7, 12), degrees=(2, 3, 4, 5, 6, 7),
                 ops=OPS):
        self.name, self.n, self.method, self.direction, self.dt, self.ops = name, n, method, direction, dt, tuple(ops)
        self.count = np.array([counts[b % len(counts)] for b in range(n)], dtype=np.uint32)
        self.degree = np.array([degrees[b % len(degrees)] for b in range(n)], dtype=np.uint32)

    def system(self):
        from ephemeris_explorer_amd.workloads import plummer
        return plummer(self.n)

    def startup(self):
        return 13 if self.method == "Stormer13" else 12

    def periods(self):
        return np.array([trigger_period(self.dt, int(c)) for c in self.count], dtype=np.int64)


def trigger_period(dt, count):
    """after how many `last_sample_time += dt` does `last_sample_time == dt * count` hold: `count` when the sum is exact, else 0 (never)"""
    s, period = 0.0, dt * float(count)
    for k in range(1, 2 * count + 65):
        s += dt
        if s == period:
            return k
        if s > period:
            return 0
    return 0


SCENES = [Scenario("p130", 130), Scenario("p330", 330), Scenario("p705", 705),
          Scenario("p330-stormer13", 330, method="Stormer13"),
          Scenario("p330-backward", 330, direction=BACKWARD),
          Scenario("p330-m0", 330, dt=0.7, counts=(3, 10, 1, 7), degrees=(3, 4, 5, 6, 7), ops=OPS_M0)]

# nothing forced: 12 + 50 steps in three uneven calls
OPS_DISPATCH = (("step_n", 7), ("step_n", 24), ("step_n", 31), ("take",))
DISPATCH = [Scenario("d530", 530, counts=(1, 2, 3), ops=OPS_DISPATCH),               # <L, 4>
            Scenario("d1030", 1030, counts=(1, 2, 3), ops=OPS_DISPATCH),             # <L, 8, DUO>
            Scenario("d2100", 2100, counts=(1, 2), ops=(("step_n", 12), ("step_n", 20), ("take",)))]      # <L, 16>, as shipped

# the target partition: every rank starts the whole system up, shards after the first operation and steps on. Only a sharded handle
# (or one of at most 64 bodies) predicts the next level in a launch of its own at the start of a batch, so only there has a batch's
# last step do_predict == false: the batches end on steps 82, 83 (a batch of one step) and 96, and the take at 96 = 8 * 12 steps
# has fitted every sample of the bodies with counts 1, 2, 3 and 12, the ones stored by those last steps included.
SHARD = Scenario("s705", 705, ops=(("step_n", 12), ("step_n", 70), ("step_n", 1), ("step_n", 13), ("take",)))


def by_name(name):
    return {s.name: s for s in SCENES + DISPATCH + [SHARD]}[name]


def _ok(st, what):
    assert st in (None, 0), what                   # the oracle returns a status, the product raises


def _solution_arrays(sol, n):
    """a Vec<UniformSpline> as arrays: (start, interval)[n, 2], npoly[n], ncoef[sum npoly], coefficients[sum npoly, 8, 3]"""
    info, npoly, nc, co = np.zeros((n, 2)), np.zeros(n, dtype=np.int64), [], []
    for b in range(n):
        start, interval, k = sol.info(b)
        info[b], npoly[b] = (start, interval), k
        c, m = sol.coeffs(b)
        co.append(np.asarray(c, dtype=np.float64).reshape(-1, 8, 3)[:k])
        nc.append(np.asarray(m, dtype=np.int32)[:k])
    return info, npoly, np.concatenate(nc), np.concatenate(co)


def run(sc, make, targets=None):
    """the scenario on make(pos, vel, mu, t0, dt, direction, count, degree, method) -> a flat dict of arrays (np.savez takes it):
         times    [rows, 6]: operation index, handle, time(), integrator_time(), step count, and for step_to its target
         take{op}_{handle}_info / _npoly / _ncoef / _coef
         final{handle}_pos / _vel / _t
    Every operation goes to every living handle (the clone joins them); `targets`: step_to's times from an earlier run, so that two
    backends are sent to the same time even where they disagree about where they are."""
    pos, vel, mu = sc.system()
    handles = [make(pos, vel, mu, 0.0, sc.dt, sc.direction, sc.count, sc.degree, sc.method)]
    out, rows, tq = {}, [], list(targets) if targets is not None else None
    for k, op in enumerate(sc.ops):
        if op[0] == "clone":
            handles.append(handles[0].clone())
        target = np.nan
        if op[0] == "step_to":
            target = tq.pop(0) if tq is not None else handles[0].integrator_time() + sc.direction * sc.dt * op[1]
        for j, h in enumerate(handles):
            where = f"{sc.name} op {k} {op} handle {j}"
            if op[0] == "step":
                _ok(h.step(), where)
            elif op[0] == "step_n":
                _ok(h.step_n(op[1]), where)
            elif op[0] == "step_to":
                _ok(h.step_to(target), where)
            elif op[0] == "take":
                for key, a in zip(("info", "npoly", "ncoef", "coef"), _solution_arrays(h.take_solution(), sc.n)):
                    out[f"take{k}_{j}_{key}"] = a
            rows.append((k, j, h.time(), h.integrator_time(), h.state()[3], target))
    out["times"] = np.array(rows, dtype=np.float64)
    for j, h in enumerate(handles):
        p, v, t, _ = h.state()
        out[f"final{j}_pos"], out[f"final{j}_vel"], out[f"final{j}_t"] = p, v, np.array([t])
    return out


def targets_of(rec):
    """step_to's targets of a recorded run, one per operation (the handles share it)"""
    t = rec["times"]
    return [float(x) for x in t[(t[:, 1] == 0) & ~np.isnan(t[:, 5]), 5]]


def run_oracle(sc, pair_variant=0, threads=1):
    """the scenario on orc.Propagator(native=True)"""
    from oracle import orc
    orc.set_pair_variant(pair_variant, native=True)
    orc.set_gravity_threads(threads, native=True)
    try:
        return run(sc, lambda *a: orc.Propagator(*a, native=True))
    finally:
        orc.set_pair_variant(0, native=True)
        orc.set_gravity_threads(1, native=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _first_body(npoly, q):
    return int(np.searchsorted(np.cumsum(npoly), q, side="right"))


def compare(got, want, label, sc):
    """every array of two runs, bit pattern against bit pattern; the message names label, scenario, operation and body"""
    assert sorted(got) == sorted(want), (label, sc.name, sorted(set(got) ^ set(want)))
    tg, tw = got["times"], want["times"]
    assert tg.shape == tw.shape, (label, sc.name, tg.shape, tw.shape)
    for rg, rw in zip(tg, tw):
        k, j = int(rw[0]), int(rw[1])
        assert np.array_equal(bits(rg[:5]), bits(rw[:5])), \
            f"{label} {sc.name}: op {k} {sc.ops[k]} handle {j}: (time, integrator_time, steps) {tuple(rg[2:5])} against {tuple(rw[2:5])}"
    order = ("info", "npoly", "ncoef", "coef")
    takes = [key[4:].split("_") for key in want if key.startswith("take")]
    for op, handle, what in sorted(takes, key=lambda t: (int(t[0]), int(t[1]), order.index(t[2]))):      # the earliest operation first
        key = f"take{op}_{handle}_{what}"
        where = f"{label} {sc.name}: op {op} {sc.ops[int(op)]} handle {handle}"
        g, w = got[key], want[key]
        if what in ("info", "npoly"):
            bad = np.flatnonzero((bits(g) != bits(w)).reshape(sc.n, -1).any(axis=1)) if g.shape == w.shape else [0]
            assert len(bad) == 0, f"{where}: body {int(bad[0])} (count {sc.count[int(bad[0])]}): {what} {g[int(bad[0])]} against {w[int(bad[0])]}"
        else:
            assert g.shape == w.shape, f"{where}: {what} {g.shape} against {w.shape}"
            bad = [] if len(w) == 0 else np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(axis=1))
            if len(bad):
                q = int(bad[0])
                b = _first_body(want[f"take{op}_{handle}_npoly"], q)
                raise AssertionError(f"{where}: body {b} (count {sc.count[b]}, degree {sc.degree[b]}): {what} of polynomial {q} of the take "
                                     f"({len(bad)} of {len(w)} differ):\n{g[q]}\nagainst\n{w[q]}")
    for key in sorted(want):
        if key.startswith("final"):
            g, w = got[key], want[key]
            bad = np.flatnonzero((bits(g) != bits(w)).reshape(len(w), -1).any(axis=1))
            assert len(bad) == 0, f"{label} {sc.name}: {key}: body {int(bad[0])}: {g[int(bad[0])]} against {w[int(bad[0])]}"
