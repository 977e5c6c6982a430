"""Scenes for k_srkn_small_many<SrknPlain> / <SrknDouble> (csrc/step_srkn_small.hip): the symplectic members of an
eph_nbody_advance_many / eph_prop_step_n_many call in one launch, a workgroup per system, every member with its own step count. Shared by
tests/test_srkn_gang_scenes.py (CPU: the conditions the scenes were planted for, on the C oracle alone) and tests/test_gpu_srkn_gang.py.
A plain module: no fixtures, no GPU import. Systems come from tests/gang_scenes.py, tables and records from tests/srkn_scenes.py.

  edges     one member per size of srkn_scenes.SIZES. Member i takes table EDGE_TABLES[i % 4] -- 15, 4, 7 and 3 stages, FSAL and not by
            turns --, the positive step at even i and the negative one (with a massless body) at odd i, and is entered ALONE after
            ENTRY[i % 3] = 0, 1 or 5 steps: the FSAL members of one launch both evaluate their first stage (0 steps taken) and carry
            it (ASR). Then EDGE_CALLS on all of them. The far member (32 bodies, one pair outside in_range() of the order it names,
            gang_scenes.far_pair) is put at index FAR_AT, not the lead: the out-of-range branch runs in a workgroup other than 0.
  stops     STOP_K = 7 steps asked of six members of one call: bounds that leave 0, 1, 3, exactly 7 and more than 7 steps, and one
            member at t0 = 1e20 whose t + h == t. Two orders of the members: the first status in member order is the underflow in
            one and the bound in the other.
  clones    four distinct entry states (a 3-body member after 0, 1, 2 and 5 steps) behind a gang larger than the CU count.
  sweep     the shipped 10-body system, McLachlanO4, ten days, h0 = 300 s: seven rows (two batches of five candidates), 11 475 steps
            in all."""
import numpy as np

import gang_scenes as gs
import srkn_scenes as ss

H = gs.H
INF = float("inf")
STEP_SIZE_UNDERFLOW, BOUND_REACHED = 1, 3                   # include/ephemeris_amd.h

# ---- edges
EDGE_TABLES = ("BlanesMoan14A", "McLachlanO4", "BlanesMoan6B", "Ruth")      # (15, FSAL), (4, not), (7, FSAL), (3, not)
ENTRY = (0, 1, 5)
EDGE_CALLS = (1, 5, 13)
FAR_AT = 4


class EdgeMember:
    def __init__(self, member, table, entry):
        self.member, self.table, self.entry, self.name, self.n = member, table, entry, f"{member.name}/{table}/{entry}", member.n


def edge_gang(pair_variant):
    """the members of the edge gang under evaluation order `pair_variant`, in member order"""
    out = [gs.edge_member(n, 1 if i % 2 == 0 else -1) for i, n in enumerate(ss.SIZES)]
    out.insert(FAR_AT, gs.far_pair(gs.range_exponent(pair_variant)))
    return [EdgeMember(m, EDGE_TABLES[i % len(EDGE_TABLES)], ENTRY[i % len(ENTRY)]) for i, m in enumerate(out)]


def edge_steps():
    """steps a member has taken behind its entry after every ganged call"""
    return list(np.cumsum(EDGE_CALLS))


# ---- per-member stops
STOP_K = 7
STOP_TABLE = "BlanesMoan6B"


class StopMember:
    """a 3-body system that stops after `steps` of the STOP_K steps asked with `status` (0: it takes them all)"""

    def __init__(self, name, n, bound_steps, t0=0.0):
        pos, vel, mu = gs.random_system(n)
        self.member = gs.Member(name, pos, vel, mu, H, t0)
        self.name, self.n = name, n
        # t >= bound is tested in front of every step: a bound half a step behind step s stops the handle after s steps
        self.bound = INF if bound_steps is None else t0 + (bound_steps - 0.5) * H if bound_steps else t0
        if t0 != 0.0:
            self.steps, self.status = 0, STEP_SIZE_UNDERFLOW
        elif bound_steps is None or bound_steps >= STOP_K:
            self.steps, self.status = STOP_K, 0
        else:
            self.steps, self.status = bound_steps, BOUND_REACHED

    def make(self, cls, **kw):
        h = self.member.make(cls, STOP_TABLE, **kw)
        h.set_bound(self.bound)
        return h


def stop_members():
    return [StopMember("more", 3, STOP_K + 3), StopMember("exactly", 17, STOP_K), StopMember("underflow", 2, None, t0=1e20),
            StopMember("three", 32, 3), StopMember("one", 3, 1), StopMember("none", 10, 0)]


STOP_ORDERS = {"underflow-first": (0, 1, 2, 3, 4, 5), "bound-first": (4, 0, 5, 2, 1, 3)}
STOP_FOLLOW_UP = 4                                          # steps of the call behind the lifted bounds


def first_status(members, order):
    return next((members[j].status for j in order if members[j].status), 0)


# ---- above the CU count
CLONE_ENTRIES = (0, 1, 2, 5)
CLONE_K = 7
CLONE_TABLE = "Pefrl"


def clone_source():
    return gs.edge_member(3, 1)


# ---- the convergence sweep
SWEEP = dict(system="simple_solar_system_2433282.5", method="McLachlanO4", days=10.0, h0=300.0)
SWEEP_STEP_LIMIT = 200000


def sweep_steps(rows, span, h0):
    """steps of the whole sweep: the truth run's and every row's"""
    return int(span / (h0 / 2.0) + sum(span / r[0] for r in rows))
