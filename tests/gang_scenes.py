"""Scenes for k_lm_small (csrc/step_small.hip on the frame of csrc/small_frame.h) at the sizes and in the forms that the shipped systems
never reach, shared by tests/test_gang_scenes.py (CPU: the conditions the scenes were planted for, on the C oracle alone) and
tests/test_gpu_gang_edges.py (every form of the kernel against the C oracle). A plain module: no fixtures, no GPU import.

A scene is data plus a `run()` that plays it on anything with the integrator's or the propagator's methods (orc.NBody /
ephemeris_explorer_amd.NBodyIntegration, orc.Propagator / ephemeris_explorer_amd.NBodyPropagator). What is planted, and for what:

  SIZES     1 (no pair at all: sP is filled from pos_cur[n - 1]), 2, 3; 10 | 11 and 21 | 22 (6 n threads carry the chains: the owner
            threads spill into a second and a third wave); 16 | 17 (the row the chains walk grows from 16 to 32 doubles); 23 | 24
            (276 pairs at 24: the first 20 live SECOND pairs of the four-wave form, `tid + 256 < npairs`), 25, 31 (some lanes' second
            pair live, some not, inside one wave) and 32 (all 240).
  masses    distinct, in [1, 1e5] (workloads.plummer's are all 1 / n: the two directed contributions of a pair could swap their masses
            unseen). The member with the NEGATIVE step of every size has one massless body (mu == 0: its contributions are signed
            zeros in the ordered sums), the one with the positive step has none.
  far pair  32 bodies, bodies 9 and 31 at -X and +X on the x axis (X = 0.99 * 2^(E / 2), E the upper exponent of in_range() of
            csrc/pair_term.h: 300 for evaluation orders 0-3, 133 for 4-6): the squared distance of THAT pair alone leaves the range of
            the wrapper-free sequences, and it is unordered pair 264 = 256 + 8: in the four-wave form the SECOND pair of lane 8 of
            wave 0, whose 64 first pairs are all in range. The mirrored scene has the far bodies at indices 0 and 1: pair 0, a
            first pair.
  desync    member i of a gang is advanced ALONE by i % L steps behind its start-up: the workgroups of one launch enter with
            different ring slots (LmArgs::cur) and step counts.
  sampled   propagators of 1, 3, 17, 24 and 32 bodies, counts [1, 2, 3, 7, 12] by body index (degrees 2 .. 7), forward and backward,
            stepped alone by different counts first: the owner threads of a gang's workgroups enter with different non-zero
            sampling phases and carried windows."""
import numpy as np

H = 60.0
SIZES = (1, 2, 3, 10, 11, 16, 17, 21, 22, 23, 24, 25, 31, 32)
METHODS = {"QuinlanTremaine12": 12, "Stormer13": 13}          # method: L (ring length = start-up steps)
FORWARD, BACKWARD = 1, -1
KDIV = 8                                                      # samples per window (sharing end points)
PAIR_THREADS_TWO = 256                                        # kSmallThreads2: the four-wave form's threads, two pairs each


# ---- what the kernel derives from n (small_frame.h / step_small.hip), restated
def npairs(n):
    return n * (n - 1) // 2


def live_second_pairs(n):
    """four-wave form: threads whose second pair `tid + 256` exists"""
    return sum(1 for tid in range(PAIR_THREADS_TWO) if tid + PAIR_THREADS_TWO < npairs(n))


def owner_waves(n):
    """waves that hold chain threads (tid < 6 n)"""
    return len({tid >> 6 for tid in range(6 * n)})


def row_length(n):
    """doubles of a row the ordered chains walk"""
    return 16 if n <= 16 else 32


def pair_index(i, j, n):
    """row-major index of the unordered pair (i < j) over the strict upper triangle (small_decode's inverse)"""
    assert 0 <= i < j < n
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def range_exponent(pair_variant):
    """E of in_range(): n2 in [2^-E, 2^E) takes the wrapper-free sequences (csrc/pair_term.h)"""
    return 300 if pair_variant <= 3 else 133


def out_of_range_pairs(pos, E):
    """indices of the unordered pairs whose squared distance, formed as the kernel forms it, fails in_range()"""
    pos = np.asarray(pos, dtype=np.float64)
    n, out = len(pos), []
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy, dz = pos[j] - pos[i]
            n2 = dx * dx + dy * dy + dz * dz
            if not (2.0 ** -E <= n2 < 2.0 ** E):
                out.append(pair_index(i, j, n))
    return out


# ---- members
class Member:
    """one system of a gang: n bodies, a signed step"""

    def __init__(self, name, pos, vel, mu, h, t0=0.0):
        self.name, self.pos, self.vel, self.mu, self.h, self.t0, self.n = name, pos, vel, mu, float(h), float(t0), len(mu)

    def make(self, cls, method, **kw):
        """cls(pos, vel, mu, t0, h, method): orc.NBody or NBodyIntegration"""
        return cls(self.pos, self.vel, self.mu, self.t0, self.h, method, **kw)


def random_system(n):
    """positions ~1e7, velocities ~1, distinct mu in [1, 1e5], seeded by n (random_system of tests/test_gpu_edge_cases.py)"""
    rng = np.random.default_rng(n)
    return rng.normal(size=(n, 3)) * 1e7, rng.normal(size=(n, 3)), rng.uniform(1.0, 1e5, size=n)


def edge_member(n, sign):
    pos, vel, mu = random_system(n)
    if sign < 0:
        mu[n // 2] = 0.0
    return Member(f"n{n}{'+' if sign > 0 else '-'}", pos, vel, mu, sign * H)


def edge_members(sign):
    return [edge_member(n, sign) for n in SIZES]


FAR_I, FAR_J = 9, 31


def far_pair(E, mirrored=False):
    """the 32-body system with ONE pair out of in_range(): (9, 31), pair 264 -- mirrored: (0, 1), pair 0"""
    pos, vel, mu = random_system(32)
    X = 0.99 * 2.0 ** (E / 2.0)
    pos[FAR_I] = (-X, 3.0e6, -2.0e6)
    pos[FAR_J] = (X, -1.0e6, 4.0e6)
    vel[FAR_I] = vel[FAR_J] = 0.0
    if mirrored:
        order = np.arange(32)
        order[[0, FAR_I]] = order[[FAR_I, 0]]
        order[[1, FAR_J]] = order[[FAR_J, 1]]
        pos, vel, mu = pos[order], vel[order], mu[order]
    return Member(f"far{'-mirrored' if mirrored else ''}-E{E}", pos, vel, mu, H)


def far_pair_index(mirrored):
    return pair_index(0, 1, 32) if mirrored else pair_index(FAR_I, FAR_J, 32)


def far_members(E):
    return [far_pair(E), far_pair(E, mirrored=True)]


# ---- the desynchronised gang
def desync_steps(i, L):
    """steps member i takes alone behind its start-up, before the first ganged call"""
    return i % L


def gang_calls(L):
    """the k of the ganged calls: inside one turn of the ring, a whole turn, one more, more than two"""
    return (1, 5, L, L + 1, 2 * L + 5)


def entry_slots(count, L):
    """ring position (steps taken mod L; LmArgs::cur is a bijection of it) of every member at every ganged call"""
    out, done = [], 0
    for k in gang_calls(L):
        out.append([(L + desync_steps(i, L) + done) % L for i in range(count)])
        done += k
    return out


def integration_record(h):
    """what is compared of an integration: positions, velocities, accelerations, (time, step count)"""
    p, v, t, c = h.state()
    return dict(pos=np.array(p), vel=np.array(v), acc=np.array(h.acc()), t=np.array([t]), steps=np.array([c], dtype=np.int64))


def _ok(st, what):
    assert st in (None, 0), what                   # the oracle returns a status, the product raises


def run_gang(members, method, make, advance_many=None, probes=()):
    """the desynchronised gang: every member started up alone (L steps), member i advanced alone by desync_steps(i, L), then
    gang_calls(L) on all of them -- through advance_many(handles, k) where given, else advance(k) on each. Returns
    (handles, records): records[0][i] = integration_record of member i on entry, records[c + 1][i] after ganged call c.
    `probes`: handle indices (not 0, the lead) that must have been members of ONE launch in every call (LaunchProbe)."""
    L = METHODS[method]
    handles = [m.make(make, method) for m in members]
    for i, (m, h) in enumerate(zip(members, handles)):
        _ok(h.advance(L), f"{m.name}: start-up")
        if desync_steps(i, L):
            _ok(h.advance(desync_steps(i, L)), f"{m.name}: alone")
    records = [[integration_record(h) for h in handles]]
    watch = {j: LaunchProbe(handles[j]) for j in probes}
    for c, k in enumerate(gang_calls(L)):
        if advance_many is not None:
            advance_many(handles, k)
        else:
            for m, h in zip(members, handles):
                _ok(h.advance(k), f"{m.name}: call {c}")
        for j, p in watch.items():
            p.assert_ganged(f"gang of {len(members)}, call {c}, handle {j} ({members[j].name})")
        records.append([integration_record(h) for h in handles])
    return handles, records


class Oracle:
    """orc.NBody runs of the members, computed once and shared: record(member, method, steps) = integration_record after `steps`
    steps from the start (one advance(1) at a time: the integrator is a state machine, the bits are those of advance(steps)).
    Members are told apart by name. The evaluation order is orc's, set by the caller (orc.set_pair_variant)."""

    def __init__(self):
        self.trails = {}

    def record(self, member, method, steps):
        key = (member.name, method)
        if key not in self.trails:
            from oracle import orc
            o = member.make(orc.NBody, method)
            self.trails[key] = (o, [integration_record(o)])
        o, trail = self.trails[key]
        while len(trail) <= steps:
            _ok(o.advance(1), f"oracle: {member.name} step {len(trail)}")
            trail.append(integration_record(o))
        return trail[steps]


def expected_gang(members, method, oracle):
    """run_gang's records, from the oracle's trails"""
    L, out, done = METHODS[method], [], 0
    for k in (0,) + gang_calls(L):
        done += k
        out.append([oracle.record(m, method, L + desync_steps(i, L) + done) for i, m in enumerate(members)])
    return out


class LaunchProbe:
    """Was a ganged call ONE launch for this member? An observable of the existing ABI, as it is today (nothing is exported for
    it): a member that is not the gang's lead and has enable_timing() on opens no event pair of its own -- the shared launch is
    timed by the lead alone (gang_frame, nbody.cpp) -- but counts the launch (commit_gang): kernel_time() keeps its milliseconds
    EXACTLY and its launch count rises by one. Where advance_many / step_n_many fall back to separate advances the member times
    its own launch and the milliseconds grow."""

    def __init__(self, handle):
        self.h = handle
        handle.enable_timing(True)
        self.ms, self.launches = handle.kernel_time()

    def after_call(self):
        """(milliseconds gained, launches gained) since the last look"""
        ms, launches = self.h.kernel_time()
        gained = (ms - self.ms, launches - self.launches)
        self.ms, self.launches = ms, launches
        return gained

    def assert_ganged(self, what):
        ms, launches = self.after_call()
        assert launches == 1 and ms == 0.0, f"{what}: not a member of one shared launch: {launches} launches, {ms} ms of its own"


def padded_plan(sources, total, L):
    """(source index, steps taken alone) of the handles of a gang of `total`: the sources as run_gang enters them (start-up and
    desync_steps), then clones -- handle j a clone of source j % sources as it stands then, advanced alone by 1, 2 or 3 steps:
    every (source, steps) occurs two or three times once total >= 7 * sources"""
    plan = [(i, L + desync_steps(i, L)) for i in range(sources)]
    for j in range(sources, total):
        plan.append((j % sources, plan[j % sources][1] + 1 + (j // sources - 1) % 3))
    return plan


def run_padded(members, method, total, make, advance_many, probes=()):
    """a gang of `total` handles by padded_plan, gang_calls(L) through advance_many. Returns (plan, records): records[c][j] after
    ganged call c. `probes`: handle indices (not 0, the lead) that must have been members of ONE launch in every call."""
    L = METHODS[method]
    plan = padded_plan(len(members), total, L)
    handles = []
    for j, (src, alone) in enumerate(plan):
        if j < len(members):
            handles.append(members[j].make(make, method))
            _ok(handles[j].advance(alone), members[j].name)
        else:
            handles.append(handles[src].clone())
            _ok(handles[j].advance(alone - plan[src][1]), f"clone {j} of {members[src].name}")
    watch = {j: LaunchProbe(handles[j]) for j in probes}
    records = []
    for c, k in enumerate(gang_calls(L)):
        advance_many(handles, k)
        for j, p in watch.items():
            p.assert_ganged(f"gang of {total}, call {c}, handle {j}")
        records.append([integration_record(h) for h in handles])
    return plan, records


def compare_padded(members, method, plan, records, oracle, label):
    """handles with the same (source, steps alone) against each other, and every handle against the oracle"""
    L, done = METHODS[method], 0
    for c, k in enumerate(gang_calls(L)):
        done += k
        first = {}
        for j, key in enumerate(plan):
            where = f"{label}: after ganged call {c}, handle {j} ({members[key[0]].name}, {key[1]} steps alone)"
            if key in first:
                diff = same_record(records[c][j], records[c][first[key]])
                assert diff is None, f"{where}: {diff} differs from handle {first[key]}, entered in the same state"
                continue
            first[key] = j
            got, want = records[c][j], oracle.record(members[key[0]], method, key[1] + done)
            diff = same_record(got, want)
            if diff in ("pos", "vel", "acc"):
                bad = np.flatnonzero((bits(got[diff]) != bits(want[diff])).any(axis=1))
                where += f": {diff} of body {int(bad[0])} ({len(bad)} of {members[key[0]].n} bodies differ): " \
                         f"{got[diff][int(bad[0])]} against {want[diff][int(bad[0])]}"
            assert diff is None, where if diff in ("pos", "vel", "acc") else f"{where}: {diff} {got[diff]!r} against {want[diff]!r}"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_record(got, want):
    """None, or the first key whose bit patterns differ"""
    for key in ("t", "steps", "pos", "vel", "acc"):
        if got[key].shape != want[key].shape or not np.array_equal(bits(got[key]), bits(want[key])):
            return key
    return None


def compare_gang(members, got, want, label):
    """records of two runs of one gang, bit pattern against bit pattern; the message names label, call, member and the first body"""
    assert len(got) == len(want), (label, len(got), len(want))
    for c, (gc, wc) in enumerate(zip(got, want)):
        for m, g, w in zip(members, gc, wc):
            key = same_record(g, w)
            if key is None:
                continue
            where = f"{label}: {'on entry' if c == 0 else f'after ganged call {c - 1}'}, member {m.name}"
            if key in ("t", "steps") or g[key].shape != w[key].shape:
                raise AssertionError(f"{where}: {key} {g[key]!r} against {w[key]!r}")
            bad = np.flatnonzero((bits(g[key]) != bits(w[key])).any(axis=1))
            raise AssertionError(f"{where}: {key} of body {int(bad[0])} ({len(bad)} of {m.n} bodies differ): "
                                 f"{g[key][int(bad[0])]} against {w[key][int(bad[0])]}")


# ---- sampled gangs
SAMPLED_SIZES = (1, 3, 17, 24, 32)
COUNTS, DEGREES = (1, 2, 3, 7, 12), (2, 3, 4, 5, 6, 7)
SAMPLED_CALLS = (1, 5, 13, 97)                                # ganged step_n_many calls: 116 steps, 96 = 8 windows' samples of count 12


class SampledMember:
    def __init__(self, n, direction):
        self.n, self.direction = n, direction
        self.name = f"p{n}{'+' if direction > 0 else '-'}"
        self.pos, self.vel, self.mu = random_system(n)
        self.count = np.array([COUNTS[b % len(COUNTS)] for b in range(n)], dtype=np.uint32)
        self.degree = np.array([DEGREES[b % len(DEGREES)] for b in range(n)], dtype=np.uint32)

    def make(self, cls, method, **kw):
        """cls(pos, vel, mu, t0, dt, direction, count, degree, method): orc.Propagator or NBodyPropagator"""
        return cls(self.pos, self.vel, self.mu, 0.0, H, self.direction, self.count, self.degree, method, **kw)

    def entry_steps(self, L):
        """steps taken alone (start-up included) before the first ganged call: different for every member, and such that two
        bodies are in different non-zero phases (s % count) -- 5 mod 6 for the 3-body member (phases 1 and 2 of its counts 2, 3)"""
        if self.n == 3:
            return 17 + 6 * (self.direction < 0)
        s = L + 1 + 5 * (2 * SAMPLED_SIZES.index(self.n) + (self.direction < 0))
        while self.n > 3 and len({s % int(c) for c in self.count} - {0}) < 2:
            s += 1
        return s


def sampled_members():
    return [SampledMember(n, d) for n in SAMPLED_SIZES for d in (FORWARD, BACKWARD)]


def solution_arrays(sol, n):
    """a Vec<UniformSpline> as arrays: (start, interval)[n, 2], npoly[n], ncoef[sum npoly], coefficients[sum npoly, 8, 3]"""
    info, npoly, nc, co = np.zeros((n, 2)), np.zeros(n, dtype=np.int64), [np.zeros(0, dtype=np.int32)], [np.zeros((0, 8, 3))]
    for b in range(n):
        start, interval, k = sol.info(b)
        info[b], npoly[b] = (start, interval), k
        c, m = sol.coeffs(b)
        co.append(np.asarray(c, dtype=np.float64).reshape(-1, 8, 3)[:k])
        nc.append(np.asarray(m, dtype=np.int32)[:k])
    return dict(info=info, npoly=npoly, ncoef=np.concatenate(nc), coef=np.concatenate(co))


def sampled_record(p, n):
    rec = solution_arrays(p.take_solution(), n)
    pos, vel, t, c = p.state()
    rec.update(pos=np.array(pos), vel=np.array(vel), t=np.array([t, p.time()]), steps=np.array([c], dtype=np.int64))
    return rec


PAD_SOURCE = 2                                                # the padding of a sampled gang: clones of the 3-body forward member


def run_sampled(members, method, make, step_n_many=None, pad_to=0, probes=()):
    """every member stepped alone to its entry_steps, then SAMPLED_CALLS on all of them -- through step_n_many(props, k) where
    given, else step_n(k) on each. `pad_to`: the gang is filled up to that many propagators with clones of member PAD_SOURCE as it
    stands then, clone q stepped alone by q % 3 more steps. `probes`: indices (not 0) whose integrations must have been members
    of ONE launch in every call. Returns (records of the members, records of the first six clones)"""
    L = METHODS[method]
    props = [m.make(make, method) for m in members]
    for m, p in zip(members, props):
        _ok(p.step_n(m.entry_steps(L)), f"{m.name}: alone")
    pad = [props[PAD_SOURCE].clone() for _ in range(max(0, pad_to - len(props)))]
    for q, p in enumerate(pad):
        if q % 3:
            _ok(p.step_n(q % 3), f"clone {q}: alone")
    gang = props + pad
    watch = {j: LaunchProbe(gang[j].integration()) for j in probes}
    for c, k in enumerate(SAMPLED_CALLS):
        if step_n_many is not None:
            step_n_many(gang, k)
        else:
            for m, p in zip(members, props):
                _ok(p.step_n(k), m.name)
        for j, p in watch.items():
            p.assert_ganged(f"sampled gang of {len(gang)}, call {c}, propagator {j}")
    return [sampled_record(p, m.n) for m, p in zip(members, props)], [sampled_record(p, members[PAD_SOURCE].n) for p in pad[:6]]


def compare_sampled(members, got, want, label):
    for m, g, w in zip(members, got, want):
        for key in ("t", "steps", "info", "npoly", "ncoef", "coef", "pos", "vel"):
            where = f"{label}: member {m.name}: {key}"
            assert g[key].shape == w[key].shape, f"{where}: {g[key].shape} against {w[key].shape}"
            diff = bits(g[key]) != bits(w[key])
            if not diff.any():
                continue
            row = int(np.flatnonzero(diff.reshape(len(diff), -1).any(axis=1))[0])
            if key in ("ncoef", "coef"):
                body = int(np.searchsorted(np.cumsum(w["npoly"]), row, side="right"))
                where += f" of polynomial {row} of the take (body {body}, count {m.count[body]}, degree {m.degree[body]})"
            elif key not in ("t", "steps"):
                where += f" of body {row}"
            raise AssertionError(f"{where}:\n{g[key][row]}\nagainst\n{w[key][row]}")
