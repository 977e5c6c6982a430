"""Scenes for k_srkn_small / k_srkn_double_small (csrc/step_srkn_small.hip on the frame of csrc/small_frame.h): the eight symplectic
Runge-Kutta-Nystrom tables on systems of at most 32 bodies, shared by tests/test_srkn_scenes.py (CPU: the C oracle pinned to
pyoracle's Srkn, and the conditions the scenes were planted for) and tests/test_gpu_srkn_small.py (the kernels against the C oracle
and against the per-stage launches). A plain module: no fixtures, no GPU import. Systems come from tests/gang_scenes.py.

  SIZES     1 (no pair: the rows stay zero, the acceleration is +0.0), 2, 3; 10 | 11 and 21 | 22 (the 6 n chain threads spill into a
            second and a third wave); 16 | 17 (the row the chains walk grows from 16 to 32 doubles); 31 and 32.
  signs     sizes alternate between the positive step (distinct masses, none zero) and the negative step (one massless body,
            gang_scenes.edge_member); 17 and 32 bodies come with both.
  far pair  gang_scenes.far_members: 32 bodies with ONE pair outside in_range() of csrc/pair_term.h.
  OPS       advance(1): the one step at which an FSAL table evaluates its first stage; advance(5); clone; advance(1) (a launch that
            enters with the FSAL carry of the launch before it, in ASR); advance(11) on the handle and on its clone.
  sampled   propagators of 3, 17 and 32 bodies, counts [1, 2, 3, 7] and degrees 2 .. 7 by body index, forward and backward: one step,
            step_n(5), a take with windows partly filled, a clone, step_to."""
import numpy as np

import gang_scenes as gs

H = gs.H
# table: (stages, FSAL) -- integration/src/methods.rs:20-27
TABLES = {"BlanesMoan6B": (7, True), "BlanesMoan11B": (12, True), "BlanesMoan14A": (15, True), "ForestRuth": (4, True),
          "McLachlanO4": (4, False), "McLachlanSS17": (18, True), "Pefrl": (5, True), "Ruth": (3, False)}
FSAL_TABLE, PLAIN_TABLE = "BlanesMoan6B", "McLachlanO4"      # one of each kind, where a test takes two tables
SIZES = (1, 2, 3, 10, 11, 16, 17, 21, 22, 31, 32)
OPS = (("advance", 1), ("advance", 5), ("clone", 0), ("advance", 1), ("advance_both", 11))
TOTAL_STEPS = 18


def members():
    """every size once, the sign alternating with the size's index; 17 and 32 with the other sign too"""
    out = [gs.edge_member(n, 1 if k % 2 == 0 else -1) for k, n in enumerate(SIZES)]
    out += [gs.edge_member(17, -1), gs.edge_member(32, -1)]
    assert len({m.name for m in out}) == len(out)
    return out


def far_members(pair_variant):
    return gs.far_members(gs.range_exponent(pair_variant))


def expected_evals(table, steps):
    stages, fsal = TABLES[table]
    return (stages - 1) * steps + 1 if fsal else stages * steps


def record(h):
    rec = gs.integration_record(h)
    rec["evals"] = np.array([h.eval_count()], dtype=np.int64)
    return rec


def same_record(got, want):
    """None, or the first key whose bit patterns differ"""
    diff = gs.same_record(got, want)
    if diff is None and not np.array_equal(got["evals"], want["evals"]):
        diff = "evals"
    return diff


def _ok(st, what):
    assert st in (None, 0), what                   # the oracle returns a status, the product raises


def run(member, table, make, prepare=None):
    """OPS on make(pos, vel, mu, t0, h, table) -> the records after every operation: the handle's, and from the clone on the
    clone's too (it must continue as the handle does). `prepare(handle)`: e.g. set_path, applied to the handle before its first step."""
    h = member.make(make, table)
    if prepare:
        prepare(h)
    twin, out = None, []
    for op, k in OPS:
        if op == "clone":
            twin = h.clone()
        elif op == "advance":
            _ok(h.advance(k), (member.name, table, op, k))
        else:
            _ok(h.advance(k), (member.name, table, op, k))
            _ok(twin.advance(k), (member.name, table, op, k, "clone"))
        out.append(record(h))
        if twin is not None:
            out.append(record(twin))
    return out


def compare(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        key = same_record(g, w)
        if key is None:
            continue
        where = f"{label}: record {k}"
        if key in ("t", "steps", "evals") or g[key].shape != w[key].shape:
            raise AssertionError(f"{where}: {key} {g[key]!r} against {w[key]!r}")
        bad = np.flatnonzero((gs.bits(g[key]) != gs.bits(w[key])).any(axis=1))
        raise AssertionError(f"{where}: {key} of body {int(bad[0])} ({len(bad)} of {len(g[key])} bodies differ): "
                             f"{g[key][int(bad[0])]} against {w[key][int(bad[0])]}")


class Oracle:
    """run() on orc.NBody, computed once per (member, table) and shared; the evaluation order is orc's, set by the caller"""

    def __init__(self):
        self.runs = {}

    def records(self, member, table):
        key = (member.name, table)
        if key not in self.runs:
            from oracle import orc
            self.runs[key] = run(member, table, orc.NBody)
        return self.runs[key]


# ---- sampled scenes
SAMPLED_SIZES = (3, 17, 32)
SAMPLED_TABLES = (FSAL_TABLE, PLAIN_TABLE)
COUNTS, DEGREES = (1, 2, 3, 7), (2, 3, 4, 5, 6, 7)


class SampledMember:
    def __init__(self, n, direction):
        self.n, self.direction = n, direction
        self.name = f"s{n}{'+' if direction > 0 else '-'}"
        self.pos, self.vel, self.mu = gs.random_system(n)
        self.count = np.array([COUNTS[b % len(COUNTS)] for b in range(n)], dtype=np.uint32)
        self.degree = np.array([DEGREES[b % len(DEGREES)] for b in range(n)], dtype=np.uint32)

    def make(self, cls, table):
        """cls(pos, vel, mu, t0, dt, direction, count, degree, method): orc.Propagator or NBodyPropagator"""
        return cls(self.pos, self.vel, self.mu, 0.0, H, self.direction, self.count, self.degree, table)


def sampled_members():
    """3 and 32 bodies forward, 17 backward"""
    return [SampledMember(3, gs.FORWARD), SampledMember(17, gs.BACKWARD), SampledMember(32, gs.FORWARD)]


def _look(p):
    return dict(t=np.array([p.time(), p.integrator_time()]))


def _take(p, n):
    rec = gs.solution_arrays(p.take_solution(), n)
    rec.update(_look(p))
    return rec


def run_sampled(member, table, make):
    """one step; step_n(5); a take (6 steps in: every window partly filled, 6, 3, 2 and 0 samples behind the first); a clone;
    step_to(+-100 H) on both; the final takes and states. -> list of (what, arrays)"""
    n, d = member.n, member.direction
    p = member.make(make, table)
    out = []
    _ok(p.step(), (member.name, table, "step"))
    out.append(("step", _look(p)))
    _ok(p.step_n(5), (member.name, table, "step_n"))
    out.append(("step_n(5)", _look(p)))
    out.append(("take at 6 steps", _take(p, n)))
    twin = p.clone()
    for who, q in (("original", p), ("clone", twin)):
        _ok(q.step_to(d * 100.0 * H), (member.name, table, "step_to", who))
        out.append((f"step_to, {who}", _look(q)))
        rec = _take(q, n)
        pos, vel, t, c = q.state()
        rec.update(pos=np.array(pos), vel=np.array(vel), steps=np.array([c], dtype=np.int64))
        out.append((f"final take and state, {who}", rec))
    return out


def compare_sampled(got, want, label):
    assert [w for w, _ in got] == [w for w, _ in want], label
    for (what, g), (_, w) in zip(got, want):
        assert sorted(g) == sorted(w), (label, what)
        for key in sorted(g):
            where = f"{label}: {what}: {key}"
            assert g[key].shape == w[key].shape, f"{where}: {g[key].shape} against {w[key].shape}"
            diff = gs.bits(g[key]) != gs.bits(w[key])
            if diff.any():
                row = int(np.flatnonzero(diff.reshape(len(diff), -1).any(axis=1))[0])
                raise AssertionError(f"{where}, row {row}:\n{g[key][row]}\nagainst\n{w[key][row]}")
