"""eph_craft_batch_plot_markers beside the route a caller had before it, built only from calls the library had before:
eph_craft_batch_event_counts, eph_craft_batch_events craft by craft, the first and the last knot of every craft (row 0 of eph_craft_batch_knot_slabs and
the epochs of eph_craft_batch_summary), the candidate rule on the host (numpy searchsorted per request, plain Python around it: its time is listed
on its own, and the totals are given with and without it), one eph_craft_batch_eval(per_craft = 1) per distinct reference body for the
positions and one per distinct burn frame for the state vectors, distances and TNB frames on the host (numpy, vectorised). Two sizes:

  frame    the app's frame: 8 ships (the Mars Transfer Ship with its burns) to 1951-01-01, the records of plot_segments (one
           whole-window config each, max 4000 points) as requests
  thread   the thread form: 16 384 perturbed copies over 220 d (scripts/craft_segments_timing.py's thread case), the records of
           plot_segments (max 64 points per segment) as requests

    python scripts/craft_markers_timing.py [--case frame|thread|both] [--reps R] [--out FILE.json]

Wall time: a host clock around the (synchronous) calls into buffers allocated and touched beforehand; the two routes alternate, R
repetitions each after a warm-up; median and min .. max. The two routes' records are compared once: candidates, epochs, positions,
distances and frames by bits. Kernel and host times inside the new call: EPH_TRACE_CRAFT_MARKERS=1 (calls of their own): the count
kernel with the host's scans, the fill kernel with the moves into the caller's array."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import ephemeris_explorer_amd as ea                                   # noqa: E402
from craft_plot_timing import I64P, RES, SYSTEMS, plot_view, spread, stderr_of      # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system, parse_epoch, soi_parents, soi_radii   # noqa: E402

DAY = 86400.0


def timeline_burns(burns):
    """the burn pieces of Timeline::new: (timeline index, start, frame's body), by start"""
    out, cursor, k = [], -1.7976931348623157e308, 0
    for start, end, _, ref in sorted(burns, key=lambda b: b[0]):
        if start > cursor:
            k += 1
        out.append((k, start, ref))
        cursor = end
        k += 1
    return out


def normalized(v):
    rcp = 1.0 / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v * rcp[:, None], np.isfinite(rcp) & (rcp > 0.0)


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def per_craft_eval(batch, craft, epochs, body):
    """eph_craft_batch_eval with every craft its own epochs: the state vectors of (craft[i], epochs[i]) relative to `body`"""
    order = np.argsort(craft, kind="stable")
    sorted_craft = craft[order]
    slot = np.arange(len(craft)) - np.searchsorted(sorted_craft, sorted_craft)
    at = np.full((int(slot.max()) + 1 if len(craft) else 1, batch.n), epochs[0] if len(craft) else 0.0)
    at[slot, sorted_craft] = epochs[order]
    y, inside = batch.eval(at, reference_body=body, raw=True)
    pos, vel, ok = np.zeros((len(craft), 3)), np.zeros((len(craft), 3)), np.zeros(len(craft), dtype=bool)
    pos[order], vel[order], ok[order] = y[slot, :3, sorted_craft], y[slot, 3:, sorted_craft], inside[slot, sorted_craft]
    return pos, vel, ok


def measure(name, batch, burns, requests, crafts, args):
    L, h, n = batch._L, batch._h, batch.n
    nr = len(requests)
    arr = (ea.MarkerRequest * nr)(*[ea.MarkerRequest(q["reference_body"], q["kinds"], q["first"], q["last"]) for q in requests])
    cr = np.ascontiguousarray(crafts, dtype=np.int64)
    first = np.ones(nr + 1, dtype=np.int64)
    st = L.eph_craft_batch_plot_markers(h, nr, arr, cr.ctypes.data_as(I64P), 0, None, first.ctypes.data_as(I64P))
    total = int(first[nr])
    assert st == ea.ERR_BAD_ARGUMENT and total > 0, (st, total)
    markers = np.ones(total, dtype=ea.SpacecraftBatch.MARKER)
    ref_of = np.array([q["reference_body"] for q in requests])
    kinds_of = np.array([q["kinds"] for q in requests])
    lo_of, hi_of = np.array([q["first"] for q in requests]), np.array([q["last"] for q in requests])
    pieces = {}
    kept, parts = {}, {}

    def new_way():
        assert L.eph_craft_batch_plot_markers(h, nr, arr, cr.ctypes.data_as(I64P), total, markers.ctypes.data_as(C.POINTER(ea.PlotMarker)),
                                              first.ctypes.data_as(I64P)) == 0

    def old_way():
        t0 = time.perf_counter()
        counts = batch.event_counts()
        t1 = time.perf_counter()
        ev = [batch.events(c, counts) for c in range(n)]
        t2 = time.perf_counter()
        knot0 = batch.knot_slabs(0, 1)[0][0]
        rec = batch.summary()                                  # (the last knot is the epoch the craft has reached: every accepted step leaves one)
        nk, last = rec["nknots"], rec["t"]
        t3 = time.perf_counter()
        rq, kind, index, body, when, apd = [], [], [], [], [], []
        for r in range(nr):                                    # the candidate rule, request by request
            c, k, lo, hi = int(cr[r]), int(kinds_of[r]), lo_of[r], hi_of[r]
            if c not in pieces:
                pieces[c] = timeline_burns(burns[c])
            if k & 1:
                for piece, start, ref in pieces[c]:
                    if lo <= start <= hi:
                        rq.append(r); kind.append(0); index.append(piece); body.append(ref); when.append(start); apd.append(0.0)
            (tt, tb), (at, ad, ab, ak) = ev[c]
            if k & 2:
                a, b = np.searchsorted(tt, lo, "left"), np.searchsorted(tt, hi, "right")
                for i in range(a, b):
                    rq.append(r); kind.append(1); index.append(i); body.append(int(tb[i])); when.append(tt[i]); apd.append(0.0)
            if k & 4:
                a, b = np.searchsorted(at, lo, "left"), np.searchsorted(at, hi, "right")
                for i in range(a, b):
                    rq.append(r); kind.append(3 if ak[i] else 2); index.append(i); body.append(int(ab[i])); when.append(at[i]); apd.append(ad[i])
            if k & 8 and nk[c] > 0:
                for which, t in ((4, knot0[c]), (5, last[c])):
                    if lo <= t <= hi:
                        rq.append(r); kind.append(which); index.append(0); body.append(-1); when.append(t); apd.append(0.0)
        rq, kind, body, when = np.array(rq), np.array(kind), np.array(body), np.array(when)
        t4 = time.perf_counter()
        out = np.zeros(len(rq), dtype=ea.SpacecraftBatch.MARKER)
        out["request"], out["kind"], out["index"], out["body"], out["time"], out["apsis_distance"] = rq, kind, index, body, when, apd
        craft_of, ref = cr[rq], ref_of[rq]
        for b in np.unique(ref):                               # one eval per distinct reference body
            sel = np.flatnonzero(ref == b)
            pos, _, ok = per_craft_eval(batch, craft_of[sel], when[sel], int(b))
            pos[~ok] = 0.0
            out["position"][sel] = pos
            d = np.sqrt(pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1] + pos[:, 2] * pos[:, 2])
            out["distance"][sel] = np.where(ok, d, 0.0)
            out["status"][sel] |= ok.astype(np.int32)
        t5 = time.perf_counter()
        burn = kind == 0
        for b in np.unique(body[burn]):                        # one eval per distinct burn frame, then the TNB frames
            sel = np.flatnonzero(burn & (body == b))
            pos, vel, ok = per_craft_eval(batch, craft_of[sel], when[sel], int(b))
            frame = np.zeros((len(sel), 9))
            if b < 0:
                frame[:] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
            else:
                with np.errstate(all="ignore"):
                    x, okx = normalized(vel)
                    y, oky = normalized(cross(pos, vel))
                    z, _ = normalized(cross(x, y))
                frame[:, :3], frame[:, 3:6], frame[:, 6:] = x, z, y
                ok = ok & okx & oky
            frame[~ok] = 0.0
            out["frame"][sel] = frame
            out["status"][sel] |= 2 * ok.astype(np.int32)
        t6 = time.perf_counter()
        for key, ms in (("event_counts", t1 - t0), ("events_per_craft", t2 - t1), ("bounds_knot_slabs_summary", t3 - t2),
                        ("host_selection_python", t4 - t3), ("eval_per_reference_body", t5 - t4), ("eval_and_frames_per_burn_frame", t6 - t5)):
            parts.setdefault(key, []).append(ms * 1e3)
        kept["out"] = out
        return (t4 - t3) * 1e3

    new_way()
    new_way()
    old_way()
    old = kept["out"]
    agree = {"count": len(old) == total}
    if agree["count"]:
        for field in ("request", "kind", "index", "body", "status", "time", "apsis_distance", "position", "distance", "frame"):
            agree[field] = bool(np.ascontiguousarray(old[field]).tobytes() == np.ascontiguousarray(markers[field]).tobytes())
    parts.clear()
    wall = {"new": [], "old": [], "old_without_python": []}
    trace = {"count_kernel": [], "count_host": [], "fill_kernel": [], "fill_host": []}
    for _ in range(args.reps):                                 # alternating
        t0 = time.perf_counter()
        new_way()
        wall["new"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        python_ms = old_way()
        ms = (time.perf_counter() - t0) * 1e3
        wall["old"].append(ms)
        wall["old_without_python"].append(ms - python_ms)
        os.environ["EPH_TRACE_CRAFT_MARKERS"] = "1"            # kernel times: a traced call of its own
        text = stderr_of(new_way)
        os.environ["EPH_TRACE_CRAFT_MARKERS"] = "0"
        for step in ("count", "fill"):
            found = re.search(rf"craft_markers_{step}: .* kernel_ms ([0-9.]+) host_copy_ms ([0-9.]+)", text)
            assert found, text
            trace[f"{step}_kernel"].append(float(found.group(1)))
            trace[f"{step}_host"].append(float(found.group(2)))
    kernels = [a + b for a, b in zip(trace["count_kernel"], trace["fill_kernel"])]
    per_request = np.diff(first)
    row = {"case": name, "craft": n, "requests": nr, "markers": total, "markers_per_request_max": int(per_request.max()),
           "kinds": np.bincount(markers["kind"], minlength=6).tolist(), "routes_agree": agree,
           "wall": {k: spread(v) for k, v in wall.items()}, "old_parts": {k: spread(v) for k, v in parts.items()},
           "trace": {k: spread(v) for k, v in trace.items()}, "kernel_total": spread(kernels),
           "kernel_share_of_call": float(np.median(kernels) / np.median(wall["new"]))}
    print(json.dumps(row), flush=True)
    return row


def system_to(end):
    s = load_system(SYSTEMS / "simple_solar_system_2433282.5")
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    return s, ship, ea.Ephemeris(ea.NBodyPropagator.from_system(s).propagate(end), s.mu)


def requests_of(batch, s, cap):
    cfg = {"start": s.epoch, "end": s.epoch + 400 * DAY, "tan2_angular_resolution": RES, "max_points_per_segment": cap}
    v = plot_view(s.epoch + 30 * DAY)
    view = {"camera_position": tuple(v.camera_position), "current": v.current}
    segments, plots = batch.plot_segments(view, cfg, soi_parents(s))
    return ea.marker_requests(segments, plots), segments["plot"].astype(np.int64)


def frame_case(args):
    s, ship, eph = system_to(parse_epoch("1952-01-01 00:00:00"))
    n = 8
    burns = [ship.burn_tuples(s.names)] * n
    batch = ea.SpacecraftBatch(eph, ship.start, np.tile(ship.pos, (n, 1)), np.tile(ship.vel, (n, 1)), ship.integrator,
                               ea.AdaptiveParams.default(ship.tolerance), burns, max_knots=20000).enable_events(soi_radii(s), 16, 8192)
    batch.propagate(parse_epoch("1951-01-01 00:00:00"))
    assert (batch.status()["status"] == 0).all() and (batch.event_counts()[2] == 0).all()
    return measure("frame", batch, burns, *requests_of(batch, s, 4000), args)


def thread_case(args):
    s, ship, eph = system_to(parse_epoch("1951-01-01 00:00:00"))
    n = 16384
    rng = np.random.default_rng(20261017)                      # tests/craft_cases.py: perturbed()
    pos, vel = ship.pos + rng.normal(0.0, 1.0, size=(n, 3)), ship.vel + rng.normal(0.0, 1e-4, size=(n, 3))
    pos[0], vel[0] = ship.pos, ship.vel
    burns = [ship.burn_tuples(s.names)] * n
    batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, ship.integrator, ea.AdaptiveParams.default(ship.tolerance), burns,
                               max_knots=4096).enable_events(soi_radii(s), 16, 512)
    batch.propagate(ship.start + 220 * DAY)
    assert np.isin(batch.status()["status"], (0, ea.KNOTS_FULL)).all()
    return measure("thread", batch, burns, *requests_of(batch, s, 64), args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("frame", "thread", "both"), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_markers_timing.py needs a HIP device: a timing without one says nothing")
    result = {"device": ea.device_name(), "library": str(ea.LIB_PATH.name), "reps": args.reps, "rows": []}
    if args.case in ("frame", "both"):
        result["rows"].append(frame_case(args))
    if args.case in ("thread", "both"):
        result["rows"].append(thread_case(args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    fmt = lambda d: f"{d['median_ms']:.3f} ({d['min_ms']:.3f} .. {d['max_ms']:.3f})"   # noqa: E731
    print("| case | craft | requests | markers | eph_craft_batch_plot_markers wall ms | composed route wall ms | without its Python | of which | "
          "count kernel ms | fill kernel ms | kernels / call |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in result["rows"]:
        t = r["trace"]
        parts = ", ".join(f"{name} {fmt(v)}" for name, v in r["old_parts"].items())
        print(f"| {r['case']} | {r['craft']} | {r['requests']} | {r['markers']} | {fmt(r['wall']['new'])} | {fmt(r['wall']['old'])} | "
              f"{fmt(r['wall']['old_without_python'])} | {parts} | {fmt(t['count_kernel'])} | {fmt(t['fill_kernel'])} | "
              f"{100 * r['kernel_share_of_call']:.1f} % |")


if __name__ == "__main__":
    main()
