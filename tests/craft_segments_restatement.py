"""setup_segment_plotting (ephemeris_explorer/src/analysis.rs:159-296) restated in plain Python: which plots a ship gets from its
SoiTransitions, its Timeline and an OrbitPlotConfig. A plain module (like craft_cases.py): test_craft_segments_abi.py pins it on the
CPU against record lists worked out by hand from the oracle's transitions, test_gpu_craft_segments.py holds
eph_craft_batch_plot_segments against it."""
import bisect

import numpy as np

from oracle import pyoracle as po

CAPTURE, ESCAPE, FLYBY, TRANSIT, ORBIT = range(5)            # PlotSegment in declaration order (analysis.rs:144-151)
FIELDS = ("plot", "transition", "timeline_segment", "soi_body", "reference_body", "kind", "is_burn", "overlapping", "start", "end")


def ord_max(a, b):
    """Ord::max(a, b): b unless a > b"""
    return a if a > b else b


def ord_min(a, b):
    """Ord::min(a, b): a unless a > b"""
    return a if a <= b else b


def segments_between(timeline, start, end):
    """Timeline::segments_between (ephemeris/src/propagators/spacecraft.rs:165-177) as an index range; timeline: the
    (start, end, thrust) list of pyoracle.timeline_new"""
    lo = bisect.bisect_right([s[1] for s in timeline], start)          # partition_point(seg.end <= start)
    hi = bisect.bisect_left([s[0] for s in timeline], end)             # partition_point(seg.start < end)
    return lo, hi


def plot_segments_of(p, transitions, timeline, config, parents):
    """analysis.rs:204-293 for one entry. transitions: (times, bodies); config: dict(start, end, reference_body=-1)
    -> list of records in FIELDS order"""
    times, bodies = [float(t) for t in transitions[0]], [int(b) for b in transitions[1]]
    reference = int(config.get("reference_body", -1))
    out = []
    for i, (t_i, b) in enumerate(zip(times, bodies)):
        nxt = (times[i + 1], bodies[i + 1]) if i + 1 < len(times) else None
        prev = (times[i - 1], bodies[i - 1]) if i > 0 else None
        if t_i > config["end"] or (nxt is not None and nxt[0] < config["start"]):
            continue
        b_parent = int(parents[b])                                     # -1: the root, which no transition names
        start = ord_max(t_i, config["start"])
        end = config["end"] if nxt is None else ord_min(nxt[0], config["end"])
        lo, hi = segments_between(timeline, start, end)
        is_from = prev is not None and b_parent >= 0 and prev[1] == b_parent
        is_to = nxt is not None and b_parent >= 0 and nxt[1] == b_parent
        if is_from and is_to:
            kind = FLYBY
        elif is_from:
            kind = CAPTURE
        elif is_to:
            kind = ESCAPE
        elif prev is not None or nxt is not None:
            kind = TRANSIT
        else:
            kind = ORBIT
        for k in range(lo, hi):                                        # (lo > hi: the reference's slice panics; nothing here)
            seg = timeline[k]
            s0, s1 = ord_max(seg[0], start), ord_min(seg[1], end)
            burn = int(seg[2] is not None)
            out.append((p, i, k, b, reference if reference >= 0 else b, kind, burn, 0, s0, s1))
            if kind == FLYBY and reference < 0:
                out.append((p, i, k, b, b_parent, kind, burn, 1, s0, s1))
    return out


def expected_segments(configs, crafts, transitions, burns, parents):
    """every entry of a call: configs[p] on craft crafts[p], transitions[c] = (times, bodies) as batch.events(c)[0] gives them,
    burns[c] the craft's burn tuples -> (records, first) as eph_craft_batch_plot_segments returns them"""
    timelines = {}
    records, first = [], [0]
    for p, (config, c) in enumerate(zip(configs, crafts)):
        c = int(c)
        if c not in timelines:
            timelines[c] = po.timeline_new(burns[c])
        records += plot_segments_of(p, transitions[c], timelines[c], config, parents)
        first.append(len(records))
    return records, np.array(first, dtype=np.int64)


def record_tuples(segments):
    """the record array SpacecraftBatch.plot_segments returns -> tuples in FIELDS order (Python ints and floats)"""
    return [tuple(float(r[f]) if f in ("start", "end") else int(r[f]) for f in FIELDS) for r in segments]


def same_records(got, want):
    """all ten fields, start / end by bits"""
    def key(r):
        return r[:8] + tuple(int(np.float64(x).view(np.uint64)) for x in r[8:])
    return len(got) == len(want) and all(key(g) == key(w) for g, w in zip(got, want))


def requests_of(segments, config_of):
    """the eph_plot_request dicts that draw the records: config_of(record) -> the entry's config"""
    out = []
    for r in segments:
        c = config_of(r)
        out.append({"reference_body": int(r["reference_body"]), "start": float(r["start"]), "end": float(r["end"]),
                    "bound": int(c.get("bound", 0)), "enabled": int(c.get("enabled", 1)),
                    "tan2_angular_resolution": c["tan2_angular_resolution"], "max_points": int(c["max_points_per_segment"])})
    return out
