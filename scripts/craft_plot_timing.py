"""eph_craft_batch_plot_points beside the way the library offered before for the same plots: read the craft's knots back from the batch
(eph_craft_batch_knots per craft for a handful of ships, eph_craft_batch_knot_slabs + a host transpose for a sweep) and hand them to
eph_plot_points. Two sizes:

  frame   the app's frame: 8 ships x ~13 000 knots (the Mars Transfer Ship with its burns over one year, eight times), four requests
          per ship (no reference / Sun / Earth / Mars, max_points 4000), 10-body system
  sweep   the default sweep of craft_eval_timing.py (262 144 craft x 0.25 d, full system), one plot per craft relative to the Earth,
          max_points 64

    python scripts/craft_plot_timing.py [--case frame|sweep|both] [--craft N] [--days D] [--blocks B] [--reps R] [--out FILE.json]

Wall time: a host clock around the (synchronous) calls into buffers allocated and touched beforehand. Both ways alternate inside every
block after a warm-up; median and min .. max over blocks x reps calls; the results of the two ways are compared bit for bit once.
Kernel time: device events around k_craft_plot_points, printed by the library under EPH_TRACE_CRAFT_PLOT=1 (calls of their own).
Bytes: per drawn point two knot rows (2 x 7 doubles) and, with a reference, one coefficient row (8 x 3 doubles) -- what the accepted
evaluations need; rejected trials and the search's reads are not counted -- over the kernel time against the 8 TB/s HBM figure of the
project's roofline. EPH_AMD_LIBRARY selects another build of the library (the variants of scripts/experiments/craft_plot_variants.patch)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import ephemeris_explorer_amd as ea                                   # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system, parse_epoch      # noqa: E402
from ephemeris_explorer_amd.workloads import craft_population          # noqa: E402

HBM_BYTES_PER_S = 8e12
DP, FP, I64P, I32P = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
RES = float(np.float32(1.0) * np.float32(0.000290888) * np.float32(0.7853982))      # threshold * ARC_MINUTE * fov
SYSTEMS = ROOT / "tests/golden/systems"


def stderr_of(fn):
    """what the library prints on file descriptor 2 while fn runs"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode()


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "calls": len(xs)}


class Outputs:
    def __init__(self, n_plots, cap):
        self.t, self.xyz = np.ones((n_plots, cap)), np.ones((n_plots, cap, 3), dtype=np.float32)
        self.cnt, self.st, self.fail = np.ones(n_plots, np.int64), np.ones(n_plots, np.int32), np.ones(n_plots)

    def args(self):
        return (self.t.ctypes.data_as(DP), self.xyz.ctypes.data_as(FP), self.cnt.ctypes.data_as(I64P), self.st.ctypes.data_as(I32P),
                self.fail.ctypes.data_as(DP))

    def same(self, other):
        if not (np.array_equal(self.cnt, other.cnt) and np.array_equal(self.st, other.st) and self.fail.tobytes() == other.fail.tobytes()):
            return False
        used = np.arange(self.t.shape[1])[None, :] < self.cnt[:, None]
        return self.t[used].tobytes() == other.t[used].tobytes() and self.xyz[used].tobytes() == other.xyz[used].tobytes()


def plot_view(current):
    v = ea.PlotView()
    v.camera_position[:] = [1.2e8, -3.0e8, 2.0e8]
    v.grid_matrix3[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    v.current = current
    return v


def measure(name, batch, eph, view, requests, crafts, cap, knots_old_way, args):
    """requests: [(reference_body, start, end, max_points)] per plot; knots_old_way() -> (kt, kp, kv, first[craft], count[craft]) read
    back from the batch, with its own parts timed into the dict it also returns"""
    L, h = batch._L, batch._h
    n_plots = len(requests)
    new_rq = (ea.PlotRequest * n_plots)(*[ea.PlotRequest(-1, ref, 0, 0, a, b, 0, 1, RES, mp) for ref, a, b, mp in requests])
    cr = np.ascontiguousarray(crafts, dtype=np.int64)
    out_new, out_old = Outputs(n_plots, cap), Outputs(n_plots, cap)
    parts = {}

    def new_way():
        assert L.eph_craft_batch_plot_points(h, C.byref(view), n_plots, new_rq, cr.ctypes.data_as(I64P), cap, *out_new.args()) == 0

    def old_way():
        t0 = time.perf_counter()
        kt, kp, kv, first, count = knots_old_way(parts)
        t1 = time.perf_counter()
        old_rq = (ea.PlotRequest * n_plots)(*[ea.PlotRequest(-1, ref, int(first[c]), int(count[c]), a, b, 0, 1, RES, mp)
                                              for (ref, a, b, mp), c in zip(requests, crafts)])
        t2 = time.perf_counter()
        assert L.eph_plot_points(eph._h, C.byref(view), n_plots, old_rq, len(kt), kt.ctypes.data_as(DP), kp.ctypes.data_as(DP),
                                 kv.ctypes.data_as(DP), cap, *out_old.args()) == 0
        parts.setdefault("knots_back", []).append((t1 - t0) * 1e3)
        parts.setdefault("eph_plot_points", []).append((time.perf_counter() - t2) * 1e3)
        return (t2 - t1) * 1e3                     # building the request array with knot_first / knot_count: python, not counted

    new_way()
    new_way()
    old_way()
    assert out_new.same(out_old), "the two ways disagree"
    assert (out_new.st == 0).all() and (out_new.cnt >= 2).all()
    parts.clear()
    wall = {"new": [], "old": []}
    kernel, host_copy = [], []
    for _ in range(args.blocks):
        for which in ("new", "old"):                          # alternating inside a block
            for _ in range(args.reps):
                t0 = time.perf_counter()
                skip = old_way() if which == "old" else (new_way() or 0.0)
                wall[which].append((time.perf_counter() - t0) * 1e3 - skip)
        os.environ["EPH_TRACE_CRAFT_PLOT"] = "1"              # kernel time: a traced call of its own
        text = stderr_of(new_way)
        os.environ["EPH_TRACE_CRAFT_PLOT"] = "0"
        found = re.search(r"craft_plot: .* passes (\d+) kernel_ms ([0-9.]+) host_copy_ms ([0-9.]+)", text)
        assert found, text
        kernel.append(float(found.group(2)))
        host_copy.append(float(found.group(3)))
    points = int(out_new.cnt.sum())
    with_ref = int(out_new.cnt[np.array([r[0] for r in requests]) >= 0].sum())
    needed = points * 2 * 7 * 8 + with_ref * 8 * 3 * 8
    row = {"case": name, "plots": n_plots, "capacity": cap, "points": points, "points_per_plot_max": int(out_new.cnt.max()),
           "wall": {k: spread(v) for k, v in wall.items()}, "old_parts": {k: spread(v) for k, v in parts.items()},
           "kernel": spread(kernel), "host_copy": spread(host_copy), "kernel_bytes_needed": needed}
    rate = needed / (row["kernel"]["median_ms"] * 1e-3)
    row["kernel"]["bytes_per_s"] = rate
    row["kernel"]["share_of_8TBps"] = rate / HBM_BYTES_PER_S
    print(json.dumps(row), flush=True)
    return row


def frame_case(args):
    s = load_system(SYSTEMS / "simple_solar_system_2433282.5")
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(parse_epoch("1952-01-01 00:00:00"))
    eph = ea.Ephemeris(sol, s.mu)
    n = 8
    burns = ship.burn_tuples(s.names)
    batch = ea.SpacecraftBatch(eph, ship.start, np.tile(ship.pos, (n, 1)), np.tile(ship.vel, (n, 1)), ship.integrator,
                               ea.AdaptiveParams.default(ship.tolerance), [burns] * n, max_knots=20000)
    batch.propagate(parse_epoch("1951-01-01 00:00:00"))
    nk = batch.status()["nknots"]
    assert (batch.status()["status"] == 0).all()
    refs = [-1] + [s.names.index(x) for x in ("Sun", "Earth", "Mars")]
    requests = [(ref, s.epoch, s.epoch + 400 * 86400.0, 4000) for _ in range(n) for ref in refs]
    crafts = np.repeat(np.arange(n), len(refs))
    first = np.concatenate([[0], np.cumsum(nk)[:-1]])
    kt, kp, kv = np.ones(int(nk.sum())), np.ones((int(nk.sum()), 3)), np.ones((int(nk.sum()), 3))

    def knots_old_way(parts):
        for c in range(n):                                    # one strided gather per craft, into its part of the arrays
            a, b = int(first[c]), int(first[c] + nk[c])
            assert batch._L.eph_craft_batch_knots(batch._h, c, kt[a:b].ctypes.data_as(DP), kp[a:b].ctypes.data_as(DP), kv[a:b].ctypes.data_as(DP)) == 0
        return kt, kp, kv, first, nk

    row = measure("frame", batch, eph, plot_view(s.epoch + 30 * 86400.0), requests, crafts, 4000, knots_old_way, args)
    row["knots_per_ship"] = int(nk[0])
    return row


def sweep_case(args):
    sysdir = SYSTEMS / "full_solar_system_2433282.5"
    s = load_system(sysdir)
    ship = load_ship(sysdir / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(s.epoch + (args.days + 40.0) * 86400.0)
    eph = ea.Ephemeris(sol, s.mu)
    n = args.craft
    pos, vel, _ = craft_population("transfer", n, s, ship)
    t_end = ship.start + args.days * 86400.0
    batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=int(1200 * args.days) + 64)
    batch.propagate(t_end)
    st = batch.status()
    assert (st["status"] == 0).all()
    nk = st["nknots"]
    rows = int(nk.max())
    earth = s.names.index("Earth")
    requests = [(earth, ship.start, t_end, 64)] * n
    slab_t, slab_y = np.ones((rows, n)), np.ones((rows, 6, n))
    first = np.concatenate([[0], np.cumsum(nk)[:-1]]).astype(np.int64)
    total = int(nk.sum())
    live = np.arange(rows)[None, :] < nk[:, None]                                       # [craft][k]
    kt, kp, kv = np.ones(total), np.ones((total, 3)), np.ones((total, 3))

    def knots_old_way(parts):
        t0 = time.perf_counter()
        assert batch._L.eph_craft_batch_knot_slabs(batch._h, 0, rows, slab_t.ctypes.data_as(DP), slab_y.ctypes.data_as(DP)) == 0
        t1 = time.perf_counter()
        kt[:] = slab_t.T[live]                                # craft-major concatenation of the occupied knots
        yt = slab_y.transpose(2, 0, 1)[live]                  # [knot of craft][6]
        kp[:] = yt[:, :3]
        kv[:] = yt[:, 3:]
        parts.setdefault("slab_read_back", []).append((t1 - t0) * 1e3)
        parts.setdefault("host_transpose", []).append((time.perf_counter() - t1) * 1e3)
        return kt, kp, kv, first, nk

    row = measure("sweep", batch, eph, plot_view(ship.start + 0.1 * 86400.0), requests, np.arange(n), 64, knots_old_way, args)
    row.update({"craft": n, "days": args.days, "nknots_mean": float(nk.mean()), "nknots_max": rows, "slab_bytes": rows * n * 7 * 8})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("frame", "sweep", "both"), default="both")
    ap.add_argument("--craft", type=int, default=262144)
    ap.add_argument("--days", type=float, default=0.25)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_plot_timing.py needs a HIP device: a timing without one says nothing")
    result = {"device": ea.device_name(), "library": str(ea.LIB_PATH.name), "blocks": args.blocks, "reps": args.reps, "rows": []}
    if args.case in ("frame", "both"):
        result["rows"].append(frame_case(args))
    if args.case in ("sweep", "both"):
        result["rows"].append(sweep_case(args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    fmt = lambda d: f"{d['median_ms']:.3f} ({d['min_ms']:.3f} .. {d['max_ms']:.3f})"   # noqa: E731
    print("| case | plots | points | eph_craft_batch_plot_points wall ms | knots back + eph_plot_points wall ms | of which | kernel ms | staging -> caller copy ms | kernel GB/s needed (share of 8 TB/s) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in result["rows"]:
        k = r["kernel"]
        parts = ", ".join(f"{name} {fmt(v)}" for name, v in r["old_parts"].items())
        print(f"| {r['case']} | {r['plots']} | {r['points']} | {fmt(r['wall']['new'])} | {fmt(r['wall']['old'])} | {parts} | {fmt(k)} | {fmt(r['host_copy'])} | "
              f"{k['bytes_per_s'] / 1e9:.2f} ({100 * k['share_of_8TBps']:.3f} %) |")


if __name__ == "__main__":
    main()
