"""eph_craft_batch_restart at the default sweep (262 144 craft of the transfer population x 0.25 d, each with one burn), against the
way the library offered the same restart before: a flight-plan edit (the burn 1 % stronger) after the propagate, then the
propagate to the plan's end.

    python scripts/craft_restart_timing.py [--craft N] [--days D] [--runs R] [--out FILE.json]

The two ways, alternating run by run, each on a batch of its own created and propagated to the plan's end beforehand (not timed):
  restart  eph_craft_batch_restart (wall, host clock around the synchronous call), then the propagate to the plan's end;
  parent   eph_timeline_divergence_time once per craft on the host (a ctypes loop: a compiled shim pays less per call, so the
           loop's time is given on its own), eph_craft_batch_eval(per_craft = 1) at the restart epochs for the knot states,
           eph_craft_batch_create from them with the new burns, the same propagate, and the read-back of both knot slabs that the
           host joins (eph_hermite_join per craft) need -- a lower bound of that path: the joins themselves come on top.
Kernel time of the sweeps that follow: eph_craft_batch_kernel_time around the propagate, restarted batch (its craft keep their deal
to the lanes from creation) against the fresh batch (dealt at its creation, from the restart states). k_craft_restart's own time
comes from a rocprofv3 --kernel-trace --stats run of this script (profiles/craft_restart.md)."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import ephemeris_explorer_amd as ea                                   # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system      # noqa: E402
from ephemeris_explorer_amd.workloads import craft_population          # noqa: E402

DP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--craft", type=int, default=262144)
    ap.add_argument("--days", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_restart_timing.py needs a HIP device: a timing without one says nothing")
    sysdir = ROOT / "tests/golden/systems/full_solar_system_2433282.5"
    s = load_system(sysdir)
    ship = load_ship(sysdir / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(s.epoch + (args.days + 40.0) * 86400.0)
    eph = ea.Ephemeris(sol, s.mu)
    n = args.craft
    pos, vel, _ = craft_population("transfer", n, s, ship)
    t_end = ship.start + args.days * 86400.0
    max_knots = int(1200 * args.days) + 64
    earth = s.names.index("Earth")
    burn = (ship.start + 0.4 * args.days * 86400.0, ship.start + 0.4 * args.days * 86400.0 + 60.0, np.array([0.0, 0.0, 1e-3]), earth)
    edited = (burn[0], burn[1], burn[2] * 1.01, earth)
    old = [[burn]] * n
    nb, bs, be, ba, br = ea._burn_arrays([burn])
    _, ns, ne, na, nr = ea._burn_arrays([edited])
    L = ea._lib()
    params = ea.AdaptiveParams.default()

    def propagated():
        b = ea.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", params, old, max_knots=max_knots)
        b.propagate(t_end)
        b.summary()                                           # the first read-back after creations (see eph_craft_batch_summary)
        return b

    result = {"craft": n, "days": args.days, "device": ea.device_name(), "runs": args.runs, "rows": {}}
    wall = {k: [] for k in ("restart", "parent_total", "parent_divergence_loop", "parent_eval", "parent_create", "parent_read_back")}
    sweep = {"restarted": [], "fresh": []}
    slab_t, slab_y = np.ones((max_knots, n)), np.ones((max_knots, 6, n))
    old_p = (ea._p(bs), ea._p(be), ea._p(ba), ea._p(br, I32P))
    new_p = (ea._p(ns), ea._p(ne), ea._p(na), ea._p(nr, I32P))
    out = C.c_double()
    out_p = C.byref(out)
    at = np.empty((1, n))
    # the new plans as the C ABI takes them, built once: both ways are timed from the C calls on (no Python list flattening)
    off = np.arange(n + 1, dtype=np.int64)
    cs, ce = np.full(n, edited[0]), np.full(n, edited[1])
    ca, cr = np.tile(edited[2], n), np.full(n, earth, dtype=np.int32)
    csr = (ea._p(off, C.POINTER(C.c_int64)), ea._p(cs), ea._p(ce), ea._p(ca), ea._p(cr, I32P))
    epoch, outcome = np.empty(n), np.empty(n, dtype=np.int32)

    def wrap(h):
        w = object.__new__(ea.SpacecraftBatch)
        w._L, w.ephemeris, w.n, w.params, w._h = L, eph, n, params, h
        return w
    for run in range(args.runs + 1):                          # run 0: warm-up of both ways, not recorded
        for way in (("restart", "parent") if run % 2 == 0 else ("parent", "restart")):
            b = propagated()
            if way == "restart":
                t0 = time.perf_counter()
                assert L.eph_craft_batch_restart(b._h, None, *csr, None, None, ea._p(epoch), ea._p(outcome, I32P)) == 0
                t1 = time.perf_counter()
                assert (outcome == 0).all()
                k0 = b.kernel_ms()
                b.propagate(t_end)
                if run:
                    wall["restart"].append((t1 - t0) * 1e3)
                    sweep["restarted"].append(b.kernel_ms() - k0)
                continue
            nk = b.status()["nknots"]
            rows = int(nk.max())
            t_a = time.perf_counter()
            before = b.state()["t"]                           # trajectory.end(): the last knot (plan end: +inf)
            for i in range(n):                                # Timeline::divergence_time_before, one call per craft
                assert L.eph_timeline_divergence_time(nb, *old_p, nb, *new_p, float(before[i]), out_p) == 0
                at[0, i] = max(out.value, ship.start)
            t_b = time.perf_counter()
            y, inside = b.eval(at, raw=True)                  # the knot states at the restart epochs
            assert inside.all()
            t_c = time.perf_counter()
            t0s, p0 = np.ascontiguousarray(at[0]), np.ascontiguousarray(y[0, :3].T)
            v0 = np.ascontiguousarray(y[0, 3:].T)
            h_ = C.c_void_p()
            assert L.eph_craft_batch_create(eph._h, n, ea._p(t0s), ea._p(p0), ea._p(v0), b"Verner87", C.byref(params), *csr, max_knots,
                                            C.byref(h_)) == 0
            fresh = wrap(h_)
            t_d = time.perf_counter()
            k0 = fresh.kernel_ms()
            fresh.propagate(t_end)
            k1 = fresh.kernel_ms()
            t_e = time.perf_counter()
            nk_f = fresh.status()["nknots"]
            assert L.eph_craft_batch_knot_slabs(b._h, 0, rows, slab_t.ctypes.data_as(DP), slab_y.ctypes.data_as(DP)) == 0
            assert L.eph_craft_batch_knot_slabs(fresh._h, 0, int(nk_f.max()), slab_t.ctypes.data_as(DP), slab_y.ctypes.data_as(DP)) == 0
            t_f = time.perf_counter()
            if run:
                # the parent's path without its propagate (the propagate is the same sweep on both sides, compared by kernel time)
                wall["parent_total"].append(((t_d - t_a) + (t_f - t_e)) * 1e3)
                wall["parent_divergence_loop"].append((t_b - t_a) * 1e3)
                wall["parent_eval"].append((t_c - t_b) * 1e3)
                wall["parent_create"].append((t_d - t_c) * 1e3)
                wall["parent_read_back"].append((t_f - t_e) * 1e3)
                sweep["fresh"].append(k1 - k0)
            del fresh, b
        print(json.dumps({"run": run, **{k: v[-1] for k, v in wall.items() if v}, **{f"sweep_{k}": v[-1] for k, v in sweep.items() if v}}), flush=True)
    result["rows"] = {**{k: spread(v) for k, v in wall.items()}, **{f"sweep_kernel_{k}": spread(v) for k, v in sweep.items()}}
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print("| what | median ms | min .. max ms |")
    print("|---|---|---|")
    for k, d in result["rows"].items():
        print(f"| {k} | {d['median_ms']:.3f} | {d['min_ms']:.3f} .. {d['max_ms']:.3f} |")


if __name__ == "__main__":
    main()
