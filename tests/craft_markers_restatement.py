"""The markers of a ship's plots restated in plain Python: plot_manoeuvre_markers, plot_transition_markers, plot_apsis_markers and
plot_bounds_markers (ephemeris_explorer/src/ui/world/tooltip.rs:84-245; the picking systems of ui/world/picking.rs:256-447 walk the
same lists) as eph_craft_batch_plot_markers answers them: the candidate rule (PlotPoints::contains, ui/world/plot.rs:170-173), the
order of the records, RelativeTrajectory::position (ephemeris/src/trajectory.rs:319-325) and the TNB frame of
ReferenceFrame::transform (dynamics/spacecraft.rs:240-293). A plain module (like craft_segments_restatement.py):
test_craft_markers_abi.py pins it on the CPU against the Mars-transfer ship's lists in the C oracle, test_gpu_craft_markers.py holds
the device against it.

Inputs are what a caller had before the call existed: batch.events(c), batch.knots(c), the craft's burn tuples, and the oracle's
solution for the bodies. Trajectory evaluations are the C oracle's (orc.hermite_eval, orc.Solution.eval), the way
closest_separation_restatement.py does it; everything else is one IEEE double operation per step in the reference's order."""
import math

import numpy as np

from oracle import orc
from oracle import pyoracle as po

MANOEUVRE, TRANSITION, PERIAPSIS, APOAPSIS, START, END = range(6)
MANOEUVRES, TRANSITIONS, APSIDES, BOUNDS = 1, 2, 4, 8             # eph_marker_request.kinds
FIELDS = ("request", "kind", "index", "body", "status", "time", "position", "distance", "apsis_distance", "frame")
NO_EVENTS = ((np.zeros(0), np.zeros(0, dtype=np.int32)),
             (np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)))
ZERO3, ZERO9 = (0.0, 0.0, 0.0), (0.0,) * 9
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def contains(request, t):
    """PlotPoints::contains: inclusive at both ends"""
    return request["first"] <= t and request["last"] >= t


def craft_state_vector(knots, t):
    """CubicHermiteSpline::state_vector (its position half is ::position, a knot hit included); None outside the knots"""
    if len(knots[0]) == 0:
        return None
    r = orc.hermite_eval(knots[0], knots[1], knots[2], t)
    return None if r is None else (tuple(float(x) for x in r[0]), tuple(float(x) for x in r[1]))


def relative_position(osol, knots, reference_body, t):
    """RelativeTrajectory::position: the reference's position first (Default without a reference), then the craft's"""
    rp = ZERO3
    if reference_body >= 0:
        p = osol.eval(reference_body, t, with_velocity=False)
        if p is None:
            return None
        rp = tuple(float(x) for x in p)
    sv = craft_state_vector(knots, t)
    if sv is None:
        return None
    return (sv[0][0] - rp[0], sv[0][1] - rp[1], sv[0][2] - rp[2])


def length(p):
    """glam DVec3::length: sqrt of x*x + y*y + z*z, summed left to right"""
    return math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])


def try_normalize(v):
    """glam try_normalize as pyoracle's burn frame states it (oracle/pyoracle.py, Craft.rhs)"""
    rcp = 1.0 / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] * rcp, v[1] * rcp, v[2] * rcp) if math.isfinite(rcp) and rcp > 0.0 else None


def cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def burn_frame(osol, knots, ref, t):
    """trajectory.state_vector(t).and_then(|sv| frame.transform(t, &sv, bodies)) (tooltip.rs:105-108) -> the nine entries of TNB.0
    column major (DMat3::from_cols(x, z, y)), or None"""
    sv = craft_state_vector(knots, t)
    if sv is None:
        return None
    if ref < 0:
        return IDENTITY
    body = osol.eval(ref, t)
    if body is None:
        return None
    rp = tuple(sv[0][k] - float(body[0][k]) for k in range(3))
    rv = tuple(sv[1][k] - float(body[1][k]) for k in range(3))
    x = try_normalize(rv)
    y = try_normalize(cross(rp, rv)) if x is not None else None
    if x is None or y is None:
        return None
    xy = cross(x, y)
    rcp = 1.0 / math.sqrt(xy[0] * xy[0] + xy[1] * xy[1] + xy[2] * xy[2])      # normalize: self * self.length().recip()
    z = (xy[0] * rcp, xy[1] * rcp, xy[2] * rcp)
    return x + z + y


def markers_of(r, request, events, knots, burns, osol):
    """The records of request r: request = dict(reference_body=-1, kinds, first, last); events = batch.events(c) (NO_EVENTS for a
    batch without them); knots = batch.knots(c); burns the craft's burn tuples -> tuples in FIELDS order (position and frame as
    tuples)"""
    reference, kinds = int(request.get("reference_body", -1)), int(request["kinds"])
    (tr_t, tr_b), (ap_t, ap_d, ap_b, ap_k) = events
    found = []                                                     # (kind, index, body, time, apsis distance)
    if kinds & MANOEUVRES:
        for k, seg in enumerate(po.timeline_new(burns)):
            if seg[2] is not None and contains(request, seg[0]):
                found.append((MANOEUVRE, k, seg[2][1], seg[0], 0.0))
    if kinds & TRANSITIONS:
        found += [(TRANSITION, i, int(b), float(t), 0.0) for i, (t, b) in enumerate(zip(tr_t, tr_b)) if contains(request, float(t))]
    if kinds & APSIDES:
        found += [(APOAPSIS if k else PERIAPSIS, i, int(b), float(t), float(d))
                  for i, (t, d, b, k) in enumerate(zip(ap_t, ap_d, ap_b, ap_k)) if contains(request, float(t))]
    if kinds & BOUNDS and len(knots[0]):
        found += [(kind, 0, -1, float(t), 0.0) for kind, t in ((START, knots[0][0]), (END, knots[0][-1])) if contains(request, float(t))]
    out = []
    for kind, index, body, t, apsis_distance in found:
        status = 0
        position = relative_position(osol, knots, reference, t)
        if position is not None:
            status |= 1
        frame = burn_frame(osol, knots, body, t) if kind == MANOEUVRE else None
        if frame is not None:
            status |= 2
        out.append((r, kind, index, body, status, t, position or ZERO3, length(position) if position else 0.0, apsis_distance,
                    frame or ZERO9))
    return out


def expected_markers(requests, crafts, events, knots, burns, osol):
    """every request of a call: requests[r] on craft crafts[r]; events[c], knots[c], burns[c] per craft
    -> (records, first) as eph_craft_batch_plot_markers returns them. (A craft asked the same request twice is restated once.)"""
    records, first, seen = [], [0], {}
    for r, (request, c) in enumerate(zip(requests, crafts)):
        c = int(c)
        asked = (c, int(request.get("reference_body", -1)), int(request["kinds"]), bits(request["first"]), bits(request["last"]))
        if asked not in seen:
            seen[asked] = markers_of(r, request, events[c], knots[c], burns[c], osol)
        records += [(r,) + m[1:] for m in seen[asked]]
        first.append(len(records))
    return records, np.array(first, dtype=np.int64)


def inputs_of(batch, with_events=True):
    """what the restatement reads of a batch, craft by craft: (events[c], knots[c])"""
    nk = batch.status()["nknots"]
    knots = {c: batch.knots(c, nk[c]) for c in range(batch.n)}
    if not with_events:
        return {c: NO_EVENTS for c in range(batch.n)}, knots
    counts = batch.event_counts()
    return {c: batch.events(c, counts) for c in range(batch.n)}, knots


def record_tuples(markers):
    """the record array SpacecraftBatch.plot_markers returns -> tuples in FIELDS order (Python ints, floats and tuples of floats)"""
    return [(int(m["request"]), int(m["kind"]), int(m["index"]), int(m["body"]), int(m["status"]), float(m["time"]),
             tuple(float(x) for x in m["position"]), float(m["distance"]), float(m["apsis_distance"]), tuple(float(x) for x in m["frame"]))
            for m in markers]


def bits(x):
    return int(np.float64(x).view(np.uint64))


def key(record):
    """a record with every double as its bit pattern"""
    return record[:5] + (bits(record[5]),) + tuple(bits(x) for x in record[6]) + (bits(record[7]), bits(record[8])) + tuple(
        bits(x) for x in record[9])


def same_markers(got, want):
    """the integers exactly, every double by its bit pattern"""
    return len(got) == len(want) and all(key(g) == key(w) for g, w in zip(got, want))


def first_difference(got, want):
    """for a failing assertion's message"""
    for i, (g, w) in enumerate(zip(got, want)):
        if key(g) != key(w):
            return i, g, w
    return min(len(got), len(want)), len(got), len(want)
