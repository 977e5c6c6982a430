"""eph_craft_batch_closest_separation beside the only way the library offered before for the same searches: the ternary search of
RelativeTrajectory::closest_separation_between driven from the host, every iteration one eph_craft_batch_eval(per_craft = 1,
reference_body = B) call per distinct target body with the two trial epochs of every craft (host_driven_search below; it uses
eph_craft_batch_eval only, so this script also runs on a tree without the new call and then times that route alone). Two sizes:

  frame   the app's frame: 8 ships (Mars Transfer Ship with its burns, ~13 000 knots each), one target body each
  sweep   the default sweep of craft_plot_timing.py: 262 144 craft over 0.25 days, every craft against the Earth

Both routes run in the same process, alternating inside a block, after a warm-up; every timed call ends in the stream
synchronisation the library does before it returns. Their outputs (found, time, distance, iterations, status, failed_at) are
compared bit for bit at the sizes timed, before anything is timed. The app's call: precision 0.001, max_iterations 1000,
distance_squared_at. Kernel time is not taken here: run this script once under `rocprofv3 --kernel-trace --stats -- python ...`.

    python scripts/closest_separation_timing.py [--case frame|sweep|both] [--craft N] [--days D] [--blocks B] [--reps R]
                                                [--out FILE.json] [--md FILE.md]
--md FILE.md (default profiles/closest_separation.md) receives the result as Markdown; whatever the file holds from the line
KEPT onwards (the kernels' resource usage, the kernel trace: written by hand) is kept."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import ephemeris_explorer_amd as ea                                   # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system, parse_epoch      # noqa: E402
from ephemeris_explorer_amd.workloads import craft_population          # noqa: E402

DP, U8P = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
SYSTEMS = ROOT / "tests/golden/systems"
EVAL_FAILED = 4
KEPT = "<!-- from here on: not written by scripts/closest_separation_timing.py -->"
HAS_NEW = "eph_craft_batch_closest_separation" in getattr(ea, "ABI_SYMBOLS", [])


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "calls": len(xs)}


def host_driven_search(batch, eph, bodies, left, right, precision=0.001, max_iterations=1000):
    """closest_separation_between + PlotSeparation.distance for craft c of the batch against body bodies[c], c = 0 .. n - 1, by
    distance_squared_at, with every trajectory evaluation done by eph_craft_batch_eval: the search the reference runs (trajectory.rs:
    202-248), one numpy operation per reference operation, all craft in step. left / right: scalars or one per craft.
    -> dict of arrays found, time, distance, iterations, status, failed_at, plus evals = eph_craft_batch_eval calls made."""
    L, h, n = batch._L, batch._h, batch.n
    bodies = np.asarray(bodies, dtype=np.int64)
    distinct = [int(b) for b in np.unique(bodies)]
    nk = batch.status()["nknots"]
    rows = int(nk.max())
    slab_t = np.zeros((rows, n))
    assert L.eph_craft_batch_knot_slabs(h, 0, rows, slab_t.ctypes.data_as(DP), None) == 0
    s0, s1 = slab_t[0].copy(), slab_t[nk - 1, np.arange(n)]                  # CubicHermiteSpline::{start, end}
    info = {b: eph.info(b) for b in distinct}
    t0 = np.array([info[int(b)][0] for b in bodies])
    t1 = np.array([info[int(b)][0] + info[int(b)][1] * float(info[int(b)][2]) for b in bodies])
    start, end = np.where(t0 < s0, s0, t0), np.where(t1 < s1, t1, s1)       # Ord::max / Ord::min  trajectory.rs:283-296
    left, right = np.broadcast_to(np.asarray(left, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(right, dtype=np.float64), (n,))
    lo, hi = np.where(left < start, start, left), np.where(right < end, right, end)     # :223-224
    out = dict(found=np.zeros(n, np.uint8), time=np.zeros(n), distance=np.zeros(n), iterations=np.zeros(n, np.int32),
               status=np.zeros(n, np.int32), failed_at=np.zeros(n), evals=0)
    y, inside = np.zeros((2, 6, n)), np.zeros((2, n), np.uint8)

    def relative(at):
        """(position - body position)[m, 3, n] and Some / None [m, n] of every craft against its own body"""
        m = at.shape[0]
        rel, ok = np.zeros((m, 3, n)), np.zeros((m, n), bool)
        for b in distinct:
            assert L.eph_craft_batch_eval(h, m, at.ctypes.data_as(DP), 1, b, y.ctypes.data_as(DP), inside.ctypes.data_as(U8P)) == 0
            out["evals"] += 1
            sel = bodies == b
            rel[:, :, sel], ok[:, sel] = y[:m, :3, sel], inside[:m, sel] != 0
        return rel, ok

    def fail(which, at):
        out["status"][which], out["failed_at"][which] = EVAL_FAILED, at[which]

    active = ~(hi <= lo)                                                    # right <= left: None
    at = np.tile(s0, (2, 1))                                                # a craft that is not searching asks for its first knot
    when = np.zeros(n)
    i = 0
    while active.any():
        i += 1
        out["iterations"][active] = i
        total = hi - lo
        mid1, mid2 = lo + total / 3.0, hi - total / 3.0
        at[0], at[1] = np.where(active, mid1, s0), np.where(active, mid2, s0)
        rel, ok = relative(at)
        d2 = (rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]       # glam length_squared
        d = d2[0] - d2[1]
        bad1, bad2 = active & ~ok[0], active & ok[0] & ~ok[1]
        nan = active & ok[0] & ok[1] & np.isnan(d)                          # the library's one departure: failed_at = mid1
        fail(bad1 | nan, mid1)
        fail(bad2, mid2)
        active &= ~(bad1 | bad2 | nan)
        done = active & ((np.abs(d) < precision) | (i > max_iterations))
        when[done] = (mid1 + (mid2 - mid1) / 2.0)[done]
        active &= ~done
        out["found"][done] = 1
        positive = ~np.signbit(d)
        lo, hi = np.where(active & positive, mid1, lo), np.where(active & ~positive, mid2, hi)
    found = out["found"] != 0
    if found.any():                                                         # relative.position(time).unwrap().length()
        rel, ok = relative(np.where(found, when, s0)[None, :].copy())
        r = rel[0]
        length = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        lost = found & ~ok[0]
        fail(lost, when)
        out["found"][lost] = 0
        good = found & ok[0]
        out["time"][good], out["distance"][good] = when[good], length[good]
    return out


class NewWay:
    """the arguments of one eph_craft_batch_closest_separation call (request c = craft c, targets are bodies), kept between calls"""

    def __init__(self, batch, bodies, left, right, precision=0.001, max_iterations=1000):
        n = batch.n
        self.batch, self.n = batch, n
        left, right = np.broadcast_to(np.asarray(left, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(right, dtype=np.float64), (n,))
        self.req = (ea.SeparationRequest * n)(*[ea.SeparationRequest(-1, int(b), 0, 0, 0, 0, float(l), float(r), precision, max_iterations, 0)
                                                for b, l, r in zip(bodies, left, right)])
        self.out = dict(found=np.ones(n, np.uint8), time=np.ones(n), distance=np.ones(n), iterations=np.ones(n, np.int32),
                        status=np.ones(n, np.int32), failed_at=np.ones(n))

    def __call__(self):
        o = self.out
        assert self.batch._L.eph_craft_batch_closest_separation(
            self.batch._h, self.n, self.req, None, None, o["found"].ctypes.data_as(U8P), o["time"].ctypes.data_as(DP),
            o["distance"].ctypes.data_as(DP), o["iterations"].ctypes.data_as(C.POINTER(C.c_int32)),
            o["status"].ctypes.data_as(C.POINTER(C.c_int32)), o["failed_at"].ctypes.data_as(DP)) == 0
        return o


def same_outputs(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("found", "time", "distance", "iterations", "status", "failed_at"))


def measure(name, batch, eph, bodies, left, right, args):
    old = lambda: host_driven_search(batch, eph, bodies, left, right)       # noqa: E731
    new = NewWay(batch, bodies, left, right) if HAS_NEW else None
    want = old()                                                            # warm-up and the comparison
    if new:
        new()
        assert same_outputs(new(), want), "the two routes disagree"
    wall = {"new": [], "old": []}
    for _ in range(args.blocks):
        for which in (("new", "old") if new else ("old",)):                 # alternating inside a block
            for _ in range(args.reps):
                t0 = time.perf_counter()
                old() if which == "old" else new()
                wall[which].append((time.perf_counter() - t0) * 1e3)
    hist = Counter(int(i) for i in want["iterations"])
    row = {"case": name, "requests": int(batch.n), "found": int((want["found"] != 0).sum()), "failed": int((want["status"] != 0).sum()),
           "compared_bit_for_bit": bool(new), "wall": {k: spread(v) for k, v in wall.items() if v},
           "old_eval_calls": int(want["evals"]), "iterations_min": min(hist), "iterations_max": max(hist),
           "iterations_histogram": {str(k): hist[k] for k in sorted(hist)}}
    print(json.dumps(row), flush=True)
    return row


def frame_case(args):
    s = load_system(SYSTEMS / "simple_solar_system_2433282.5")
    ship = load_ship(SYSTEMS / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(parse_epoch("1952-01-01 00:00:00"))
    eph = ea.Ephemeris(sol, s.mu)
    n = 8
    rng = np.random.default_rng(8)
    burns = ship.burn_tuples(s.names)
    batch = ea.SpacecraftBatch(eph, ship.start, ship.pos + rng.normal(0.0, 1.0, (n, 3)), np.tile(ship.vel, (n, 1)), ship.integrator,
                               ea.AdaptiveParams.default(ship.tolerance), [burns] * n, max_knots=20000)
    batch.propagate(parse_epoch("1951-01-01 00:00:00"))
    assert (batch.status()["status"] == 0).all()
    bodies = [s.names.index(x) for x in ("Mars", "Earth", "Sun", "Moon", "Venus", "Mars", "Jupiter", "Earth")]
    row = measure("frame", batch, eph, bodies, s.epoch, s.epoch + 400 * 86400.0, args)
    row["knots_per_ship"] = int(batch.status()["nknots"][0])
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
    row = measure("sweep", batch, eph, np.full(n, s.names.index("Earth")), ship.start, t_end, args)
    row.update({"craft": n, "days": args.days, "nknots_mean": float(st["nknots"].mean()), "nknots_max": int(st["nknots"].max())})
    return row


def markdown(result):
    head = (f"# `eph_craft_batch_closest_separation` against the search driven from the host -- 1 x {result['device']}\n\n"
            "`scripts/closest_separation_timing.py`: both routes in one process, alternating inside a block "
            f"({result['blocks']} blocks x {result['reps']} calls each), after a warm-up, outputs compared bit for bit before the timing. "
            "The old route is the reference's ternary search on the host with one `eph_craft_batch_eval(per_craft = 1)` call per "
            "iteration and distinct target body. Median (min .. max), ms of wall time per search of all requests.\n\n")
    fmt = lambda d: f"{d['median_ms']:.3f} ({d['min_ms']:.3f} .. {d['max_ms']:.3f}, {d['calls']} calls)"   # noqa: E731
    lines = [head + "| case | requests | found | failed | eph_craft_batch_closest_separation wall ms | host-driven search over eph_craft_batch_eval wall ms "
             "| eph_craft_batch_eval calls per search | iterations min .. max | outputs compared bit for bit |", "|---|---|---|---|---|---|---|---|---|"]
    for r in result["rows"]:
        new = fmt(r["wall"]["new"]) if "new" in r["wall"] else "not in this library"
        lines.append(f"| {r['case']} | {r['requests']} | {r['found']} | {r['failed']} | {new} | {fmt(r['wall']['old'])} | {r['old_eval_calls']} | "
                     f"{r['iterations_min']} .. {r['iterations_max']} | {'yes' if r['compared_bit_for_bit'] else 'no'} |")
    lines.append("")
    for r in result["rows"]:
        lines.append(f"Iteration-count histogram, {r['case']} (iterations: requests): " +
                     ", ".join(f"{k}: {v}" for k, v in r["iterations_histogram"].items()))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("frame", "sweep", "both"), default="both")
    ap.add_argument("--craft", type=int, default=262144)
    ap.add_argument("--days", type=float, default=0.25)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=str(ROOT / "profiles" / "closest_separation.md"))
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("closest_separation_timing.py needs a HIP device: a timing without one says nothing")
    result = {"device": ea.device_name(), "library": str(ea.LIB_PATH.name), "blocks": args.blocks, "reps": args.reps, "rows": []}
    if args.case in ("frame", "both"):
        result["rows"].append(frame_case(args))
    if args.case in ("sweep", "both"):
        result["rows"].append(sweep_case(args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    md = Path(args.md)
    old = md.read_text() if md.exists() else ""
    md.parent.mkdir(parents=True, exist_ok=True)
    md.write_text(markdown(result) + ("\n" + old[old.index(KEPT):] if KEPT in old else ""))
    print(markdown(result))


if __name__ == "__main__":
    main()
