"""eph_craft_batch_plot_segments beside the route it replaces, built only from calls the library had before: eph_craft_batch_event_counts,
eph_craft_batch_events craft by craft, setup_segment_plotting restated on the host (tests/craft_segments_restatement.py, plain Python:
its time is listed on its own, and the totals are given with and without it), the eph_plot_request array built from its records and
eph_craft_batch_plot_points. Two sizes:

  frame    the app's frame: 8 ships (the Mars Transfer Ship with its burns) to 1951-01-01, one whole-window config each, max 4000 points
  thread   the thread form: 16 384 perturbed copies over 220 d (tests/test_gpu_craft_plot.py's thread_case with events on), one config
           each, max 64 points per segment

    python scripts/craft_segments_timing.py [--case frame|thread|both] [--reps R] [--out FILE.json]

Wall time: a host clock around the (synchronous) calls into buffers allocated and touched beforehand; the two routes alternate, R
repetitions each after a warm-up; median and min .. max. The records and every point row of the two routes are compared bit for bit once.
Kernel and host times inside the new call: EPH_TRACE_CRAFT_SEGMENTS=1 (calls of their own): the count kernel with the host's scan, the
fill kernel with the lane sort, the sampler with its row copies."""
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
sys.path.insert(0, str(ROOT / "tests"))

import craft_segments_restatement as R                                # noqa: E402
import ephemeris_explorer_amd as ea                                   # noqa: E402
from craft_plot_timing import DP, I32P, I64P, RES, SYSTEMS, Outputs, plot_view, spread, stderr_of      # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system, parse_epoch, soi_parents, soi_radii   # noqa: E402

DAY = 86400.0


def measure(name, batch, burns, parents, view, cfg, cap, args):
    L, h, n = batch._L, batch._h, batch.n
    configs = (ea.OrbitPlotConfig * n)(*[ea.OrbitPlotConfig(cfg["start"], cfg["end"], 0, 1, RES, cap, -1)] * n)
    par = np.ascontiguousarray(parents, dtype=np.int32)
    first = np.ones(n + 1, dtype=np.int64)
    assert L.eph_craft_batch_plot_segments(h, n, configs, None, par.ctypes.data_as(I32P), 0, None, first.ctypes.data_as(I64P), None, 0,
                                           None, None, None, None, None) == ea.ERR_BAD_ARGUMENT
    total = int(first[n])
    records = np.ones(total, dtype=ea.SpacecraftBatch.SEGMENT)
    out_new, out_old = Outputs(total, cap), Outputs(total, cap)
    timelines = {}
    kept = {}

    def new_way():
        assert L.eph_craft_batch_plot_segments(h, n, configs, None, par.ctypes.data_as(I32P), total, records.ctypes.data_as(C.POINTER(ea.PlotSegment)),
                                               first.ctypes.data_as(I64P), C.byref(view), cap, *out_new.args()) == 0

    parts = {}

    def old_way():
        t0 = time.perf_counter()
        counts = batch.event_counts()
        t1 = time.perf_counter()
        tr = [batch.events(c, counts)[0] for c in range(n)]
        t2 = time.perf_counter()
        composed = []
        for c in range(n):
            if c not in timelines:
                timelines[c] = R.po.timeline_new(burns[c])
            composed += R.plot_segments_of(c, tr[c], timelines[c], cfg, parents)
        rq = (ea.PlotRequest * len(composed))(*[ea.PlotRequest(-1, r[4], 0, 0, r[8], r[9], 0, 1, RES, cap) for r in composed])
        crafts = np.array([r[0] for r in composed], dtype=np.int64)
        t3 = time.perf_counter()
        assert L.eph_craft_batch_plot_points(h, C.byref(view), len(composed), rq, crafts.ctypes.data_as(I64P), cap, *out_old.args()) == 0
        t4 = time.perf_counter()
        for key, ms in (("event_counts", t1 - t0), ("events_per_craft", t2 - t1), ("host_composition_python", t3 - t2),
                        ("eph_craft_batch_plot_points", t4 - t3)):
            parts.setdefault(key, []).append(ms * 1e3)
        kept["composed"] = composed
        return (t3 - t2) * 1e3

    new_way()
    new_way()
    old_way()
    assert R.same_records(R.record_tuples(records), kept["composed"]), "the two routes disagree on the records"
    assert out_new.same(out_old), "the two routes disagree on the points"
    parts.clear()
    wall = {"new": [], "old": [], "old_without_python": []}
    trace = {"count_kernel": [], "count_host": [], "fill_kernel": [], "fill_host": [], "points_kernel": [], "points_host_copy": []}
    for _ in range(args.reps):                                 # alternating
        t0 = time.perf_counter()
        new_way()
        wall["new"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        python_ms = old_way()
        ms = (time.perf_counter() - t0) * 1e3
        wall["old"].append(ms)
        wall["old_without_python"].append(ms - python_ms)
        os.environ["EPH_TRACE_CRAFT_SEGMENTS"] = "1"           # kernel times: a traced call of its own
        text = stderr_of(new_way)
        os.environ["EPH_TRACE_CRAFT_SEGMENTS"] = "0"
        for step in ("count", "fill", "points"):
            found = re.search(rf"craft_segments_{step}: .* kernel_ms ([0-9.]+) host_copy_ms ([0-9.]+)", text)
            assert found, text
            trace[f"{step}_kernel"].append(float(found.group(1)))
            trace[f"{step}_host" + ("_copy" if step == "points" else "")].append(float(found.group(2)))
    kernels = [a + b + c for a, b, c in zip(trace["count_kernel"], trace["fill_kernel"], trace["points_kernel"])]
    row = {"case": name, "craft": n, "records": total, "capacity": cap, "points": int(out_new.cnt.sum()),
           "wall": {k: spread(v) for k, v in wall.items()}, "old_parts": {k: spread(v) for k, v in parts.items()},
           "trace": {k: spread(v) for k, v in trace.items()}, "kernel_total": spread(kernels),
           "count_kernel_share_of_kernel_time": float(np.median(trace["count_kernel"]) / np.median(kernels)),
           "count_kernel_share_of_call": float(np.median(trace["count_kernel"]) / np.median(wall["new"])),
           "kinds": np.bincount(records["kind"], minlength=5).tolist(), "overlapping": int(records["overlapping"].sum())}
    print(json.dumps(row), flush=True)
    return row


def system_to(end):
    s = load_system(SYSTEMS / "simple_solar_system_2433282.5")
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    return s, ship, ea.Ephemeris(ea.NBodyPropagator.from_system(s).propagate(end), s.mu)


def frame_case(args):
    s, ship, eph = system_to(parse_epoch("1952-01-01 00:00:00"))
    n = 8
    burns = [ship.burn_tuples(s.names)] * n
    batch = ea.SpacecraftBatch(eph, ship.start, np.tile(ship.pos, (n, 1)), np.tile(ship.vel, (n, 1)), ship.integrator,
                               ea.AdaptiveParams.default(ship.tolerance), burns, max_knots=20000).enable_events(soi_radii(s), 16, 8192)
    batch.propagate(parse_epoch("1951-01-01 00:00:00"))
    assert (batch.status()["status"] == 0).all() and (batch.event_counts()[2] == 0).all()
    cfg = {"start": s.epoch, "end": s.epoch + 400 * DAY}
    return measure("frame", batch, burns, soi_parents(s), plot_view(s.epoch + 30 * DAY), cfg, 4000, args)


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
    cfg = {"start": s.epoch, "end": s.epoch + 400 * DAY}
    return measure("thread", batch, burns, soi_parents(s), plot_view(s.epoch + 30 * DAY), cfg, 64, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("frame", "thread", "both"), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_segments_timing.py needs a HIP device: a timing without one says nothing")
    result = {"device": ea.device_name(), "library": str(ea.LIB_PATH.name), "reps": args.reps, "rows": []}
    if args.case in ("frame", "both"):
        result["rows"].append(frame_case(args))
    if args.case in ("thread", "both"):
        result["rows"].append(thread_case(args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    fmt = lambda d: f"{d['median_ms']:.3f} ({d['min_ms']:.3f} .. {d['max_ms']:.3f})"   # noqa: E731
    print("| case | craft | records | points | eph_craft_batch_plot_segments wall ms | composed route wall ms | without its Python | of which | "
          "count kernel ms | fill kernel ms | sampler kernel ms | row copy ms | count kernel / kernel time | / call |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in result["rows"]:
        t = r["trace"]
        parts = ", ".join(f"{name} {fmt(v)}" for name, v in r["old_parts"].items())
        print(f"| {r['case']} | {r['craft']} | {r['records']} | {r['points']} | {fmt(r['wall']['new'])} | {fmt(r['wall']['old'])} | "
              f"{fmt(r['wall']['old_without_python'])} | {parts} | {fmt(t['count_kernel'])} | {fmt(t['fill_kernel'])} | {fmt(t['points_kernel'])} | "
              f"{fmt(t['points_host_copy'])} | {100 * r['count_kernel_share_of_kernel_time']:.2f} % | {100 * r['count_kernel_share_of_call']:.3f} % |")


if __name__ == "__main__":
    main()
