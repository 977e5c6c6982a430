"""eph_craft_batch_eval at the default sweep (262 144 craft x 0.25 d, after propagate): wall time and kernel time of the call for
m = 1, 16, 64 ascending shared epochs relative to the Earth, beside what the library offered for the same answer before: the read-back
of the occupied knot slab (eph_craft_batch_knot_slabs; a lower bound of the old route -- one eph_hermite_eval call per craft came on
top). (The version of this script that also timed a per-lane cursor galloping over the ascending grid, and the kernel it timed, are
in scripts/experiments/craft_eval_gallop.patch; the numbers in profiles/craft_eval.md.)

    python scripts/craft_eval_timing.py [--craft N] [--days D] [--blocks B] [--reps R] [--out FILE.json]

Wall time: a host clock around the (synchronous) call into buffers allocated and touched beforehand. Kernel time: device events around
k_craft_eval, printed by the library under EPH_TRACE_CRAFT_EVAL=1 (calls of their own, not the ones timed by the host clock). The new
call and the read-back alternate inside every block; median and min .. max over blocks x reps calls. Bytes: per (craft, epoch) two knot
rows read (2 x 7 doubles) and one result row written (6 doubles + 1 byte) -- what the algorithm needs, the search's reads not counted --
over the kernel time, against the 8 TB/s HBM figure of the project's roofline."""
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
from ephemeris_explorer_amd.systems import load_ship, load_system      # noqa: E402
from ephemeris_explorer_amd.workloads import craft_population          # noqa: E402

HBM_BYTES_PER_S = 8e12
DP, U8P = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--craft", type=int, default=262144)
    ap.add_argument("--days", type=float, default=0.25)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_eval_timing.py needs a HIP device: a timing without one says nothing")
    sysdir = ROOT / "tests/golden/systems/full_solar_system_2433282.5"
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
    earth = s.names.index("Earth")
    L, h = batch._L, batch._h
    result = {"craft": n, "days": args.days, "nknots_mean": float(nk.mean()), "nknots_max": int(nk.max()), "device": ea.device_name(),
              "blocks": args.blocks, "reps": args.reps, "rows": []}

    # the old route's read-back: the occupied knots of every craft, into touched buffers
    rows = int(nk.max())
    slab_t, slab_y = np.ones((rows, n)), np.ones((rows, 6, n))

    def read_back():
        assert L.eph_craft_batch_knot_slabs(h, 0, rows, slab_t.ctypes.data_as(DP), slab_y.ctypes.data_as(DP)) == 0

    for m in (1, 16, 64):
        at = np.linspace(ship.start + 30.0, t_end - 30.0, m) if m > 1 else np.array([0.5 * (ship.start + t_end)])
        y, inside = np.ones((m, 6, n)), np.ones((m, n), dtype=np.uint8)

        def evaluate():
            assert L.eph_craft_batch_eval(h, m, at.ctypes.data_as(DP), 0, earth, y.ctypes.data_as(DP), inside.ctypes.data_as(U8P)) == 0

        wall = {"eval": [], "read_back": []}
        kernel, host_copy, passes = [], [], 0
        evaluate()                                            # warm-up of every shape
        evaluate()
        assert inside.all()
        read_back()
        for _ in range(args.blocks):
            for name in ("eval", "read_back"):                # alternating inside a block
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    read_back() if name == "read_back" else evaluate()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            os.environ["EPH_TRACE_CRAFT_EVAL"] = "1"          # kernel time: a traced call of its own
            text = stderr_of(evaluate)
            os.environ["EPH_TRACE_CRAFT_EVAL"] = "0"
            found = re.search(r"craft_eval: .* passes (\d+) kernel_ms ([0-9.]+) host_copy_ms ([0-9.]+)", text)
            assert found, text
            passes = int(found.group(1))
            kernel.append(float(found.group(2)))
            host_copy.append(float(found.group(3)))
        needed = m * n * (2 * 7 * 8 + 6 * 8 + 1)
        row = {"m": m, "passes": passes, "result_bytes": m * n * 49, "read_back_bytes": rows * n * 7 * 8, "kernel_bytes_needed": needed,
               "wall": {k: spread(v) for k, v in wall.items()}, "kernel": spread(kernel), "host_copy": spread(host_copy)}
        rate = needed / (row["kernel"]["median_ms"] * 1e-3)
        row["kernel"]["bytes_per_s"] = rate
        row["kernel"]["share_of_8TBps"] = rate / HBM_BYTES_PER_S
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print("| m | passes | result MB | eph_craft_batch_eval wall ms | knot_slabs read-back wall ms | kernel ms | staging -> caller copy ms | kernel GB/s (share of 8 TB/s) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in result["rows"]:
        w, k = r["wall"], r["kernel"]
        fmt = lambda d: f"{d['median_ms']:.3f} ({d['min_ms']:.3f} .. {d['max_ms']:.3f})"   # noqa: E731
        print(f"| {r['m']} | {r['passes']} | {r['result_bytes'] / 1e6:.0f} | {fmt(w['eval'])} | {fmt(w['read_back'])} | {fmt(k)} | {fmt(r['host_copy'])} | "
              f"{k['bytes_per_s'] / 1e9:.0f} ({100 * k['share_of_8TBps']:.1f} %) |")
    print(f"mean knots per craft {result['nknots_mean']:.1f}, max {result['nknots_max']}; read-back {result['rows'][0]['read_back_bytes'] / 1e6:.0f} MB")


if __name__ == "__main__":
    main()
