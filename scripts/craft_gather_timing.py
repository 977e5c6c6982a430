"""eph_craft_batch_gather: the kernel time of the slab move (the EPH_TRACE_GATHER lines the library prints: gather_scalars = the
per-craft arrays, gather_slabs = the knot and event slabs) and the call's wall time, beside eph_craft_batch_clone of the same batch in
the same run (hipMemcpyAsync of the whole slabs: code the gather does not touch).

  sweep   the default sweep shape: 262 144 craft x 364 knots, full slabs (one massive body at rest, every craft 363 steps), four
          selections: identity, an ordered 90 %, an ordered 3 %, a random permutation. On a dealt batch (--deal dealt, the library's
          default at this size) source and output are dealt by the same estimate of the same craft, so the slab kernel sees the
          permutation as the identity; it is the uncoalesced worst case on an undealt one (--deal undealt: EPH_CRAFT_SORT=0)
  frame   the app's frame: 8 one-ship batches (the Mars Transfer Ship to 1951-01-01, events on) gathered into one batch, and what one
          plot_segments + plot_markers pass costs on the one batch against eight passes on the eight batches
  lifecycle  eph_craft_batch_create of the sweep shape's batch and eph_craft_batch_clone of the fresh batch, wall times only

    python scripts/craft_gather_timing.py [--case sweep|frame|both|lifecycle] [--deal dealt|undealt] [--craft N] [--knots K] [--reps R]
                                          [--out FILE.json]

Per the measuring guide: one warm-up call, then the median of R >= 5 calls (min .. max beside it); needed bytes = 56 B per used knot of
the output, read and written once each. Wall times are a host clock around the synchronous call and include the allocation of the new
batch (the library clears a cached block before it hands it out), for the gather and the clone alike."""
import argparse
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
from craft_plot_timing import spread, stderr_of                       # noqa: E402

HBM_PEAK = 8.0e12                                                     # MI355X: 8 TB/s
MU = 398600.4418


def traced(fn):
    """fn() under EPH_TRACE_GATHER=1 -> (result, kernel ms of the per-craft arrays, kernel ms of the slabs, wall ms)"""
    os.environ["EPH_TRACE_GATHER"] = "1"
    box = {}

    def run():
        t0 = time.perf_counter()
        box["out"] = fn()
        box["wall"] = (time.perf_counter() - t0) * 1e3
    text = stderr_of(run)
    os.environ["EPH_TRACE_GATHER"] = "0"
    ms = {}
    for unit in ("gather_scalars", "gather_slabs"):
        found = re.search(rf"{unit}: craft \d+ sources \d+ passes \d+ kernel_ms ([0-9.]+) host_copy_ms ([0-9.]+)", text)
        assert found, text
        ms[unit] = float(found.group(1))
    return box["out"], ms["gather_scalars"], ms["gather_slabs"], box["wall"]


def timed_gather(make, reps):
    out = make()                                                      # warm-up
    del out
    rows = {"scalars_kernel": [], "slabs_kernel": [], "wall": []}
    for _ in range(reps):
        out, a, b, w = traced(make)
        del out
        rows["scalars_kernel"].append(a), rows["slabs_kernel"].append(b), rows["wall"].append(w)
    return {k: spread(v) for k, v in rows.items()}


def sweep_case(args):
    n, knots = args.craft, args.knots
    rng = np.random.default_rng(20261019)
    table = ([0.0], [2.0 ** 30], [[np.zeros((2, 3))]])                # one body at rest at the origin
    eph = ea.Ephemeris(ea.Solution.from_parts(*table), [MU])
    r = 7000.0 * 8.0 ** rng.random(n)
    ang = rng.random(n) * 2.0 * np.pi
    pos = np.stack([r * np.cos(ang), r * np.sin(ang), 0.1 * r * np.sin(3.0 * ang)], axis=1)
    v = np.sqrt(MU / r)
    vel = np.stack([-v * np.sin(ang), v * np.cos(ang), np.zeros(n)], axis=1)
    batch = ea.SpacecraftBatch(eph, 0.0, pos, vel, "Verner87", ea.AdaptiveParams.default(1e-3), max_knots=knots)
    batch.step_n(knots - 1)
    nk = batch.status()["nknots"].astype(np.int64)
    assert (nk == knots).all(), (nk.min(), nk.max())
    slab_bytes = 56 * n * knots
    selections = {"identity": np.arange(n), "ordered 90 %": np.sort(rng.choice(n, int(0.9 * n), replace=False)),
                  "ordered 3 %": np.sort(rng.choice(n, int(0.03 * n), replace=False)), "random permutation": rng.permutation(n)}
    rows = []
    clone_wall = []
    c = batch.clone()
    del c
    for _ in range(args.reps):
        t0 = time.perf_counter()
        c = batch.clone()
        clone_wall.append((time.perf_counter() - t0) * 1e3)
        del c
    clone = spread(clone_wall)
    rows.append({"case": "clone (whole slabs, wall)", "craft": n, "needed_bytes": 2 * slab_bytes, "wall": clone,
                 "bytes_per_s_wall": 2 * slab_bytes / (clone["median_ms"] * 1e-3)})
    for name, idx in selections.items():
        idx = idx.astype(np.int64)
        t = timed_gather(lambda: batch.select(idx), args.reps)
        needed = 2 * 56 * int(nk[idx].sum())
        rows.append({"case": name, "craft": len(idx), "needed_bytes": needed, **t,
                     "bytes_per_s_kernel": needed / (t["slabs_kernel"]["median_ms"] * 1e-3),
                     "bytes_per_s_wall": needed / (t["wall"]["median_ms"] * 1e-3),
                     "share_of_hbm_peak": needed / (t["slabs_kernel"]["median_ms"] * 1e-3) / HBM_PEAK})
    for row in rows:
        row["deal"] = args.deal
        print(json.dumps(row), flush=True)
    return {"shape": {"craft": n, "knots": knots, "slab_bytes": slab_bytes}, "deal": args.deal, "rows": rows}


def lifecycle_case(args):
    """create and clone on their own: the sweep shape's batch created (its knot slabs are allocated, one knot of each craft is
    written) and that fresh batch cloned (whole slabs), a host clock around each call, one warm-up of each first"""
    n, knots = args.craft, args.knots
    rng = np.random.default_rng(20261020)
    eph = ea.Ephemeris(ea.Solution.from_parts([0.0], [2.0 ** 30], [[np.zeros((2, 3))]]), [MU])
    r = 7000.0 * 8.0 ** rng.random(n)
    ang = rng.random(n) * 2.0 * np.pi
    pos = np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(n)], axis=1)
    vel = np.stack([-np.sqrt(MU / r) * np.sin(ang), np.sqrt(MU / r) * np.cos(ang), np.zeros(n)], axis=1)
    params = ea.AdaptiveParams.default(1e-3)
    wall = {"create": [], "clone": []}
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        batch = ea.SpacecraftBatch(eph, 0.0, pos, vel, "Verner87", params, max_knots=knots)
        t1 = time.perf_counter()
        c = batch.clone()
        t2 = time.perf_counter()
        del c, batch
        if rep:
            wall["create"].append((t1 - t0) * 1e3), wall["clone"].append((t2 - t1) * 1e3)
    row = {"case": "lifecycle", "craft": n, "knots": knots, **{k: spread(v) for k, v in wall.items()}}
    print(json.dumps(row), flush=True)
    return row


def frame_case(args):
    from craft_markers_timing import system_to
    from ephemeris_explorer_amd.systems import parse_epoch, soi_parents, soi_radii
    from craft_plot_timing import RES, plot_view
    s, ship, eph = system_to(parse_epoch("1952-01-01 00:00:00"))
    n = 8
    burns = ship.burn_tuples(s.names)
    ones = []
    for i in range(n):
        b = ea.SpacecraftBatch(eph, ship.start, ship.pos[None, :], ship.vel[None, :], ship.integrator,
                               ea.AdaptiveParams.default(ship.tolerance), [burns], max_knots=20000).enable_events(soi_radii(s), 16, 8192)
        b.propagate(parse_epoch("1951-01-01 00:00:00"))
        ones.append(b)
    knots = [int(b.status()["nknots"][0]) for b in ones]
    t = timed_gather(lambda: ea.SpacecraftBatch.concat(ones), args.reps)
    fleet = ea.SpacecraftBatch.concat(ones)
    cfg = {"start": s.epoch, "end": s.epoch + 400 * 86400.0, "tan2_angular_resolution": RES, "max_points_per_segment": 4000}
    v = plot_view(s.epoch + 30 * 86400.0)
    view = {"camera_position": tuple(v.camera_position), "current": v.current}
    parents = soi_parents(s)

    def one_pass(batch):
        segments, plots = batch.plot_segments(view, cfg, parents)
        return batch.plot_markers(ea.marker_requests(segments, plots), segments["plot"].astype(np.int64))
    one_pass(fleet)
    for b in ones:
        one_pass(b)
    wall = {"one batch of 8": [], "8 batches of one": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        one_pass(fleet)
        wall["one batch of 8"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for b in ones:
            one_pass(b)
        wall["8 batches of one"].append((time.perf_counter() - t0) * 1e3)
    needed = 2 * 56 * sum(knots)
    row = {"case": "frame", "ships": n, "knots": knots, "needed_bytes": needed, **t,
           "bytes_per_s_kernel": needed / (t["slabs_kernel"]["median_ms"] * 1e-3),
           "plot_segments_and_markers_wall": {k: spread(x) for k, x in wall.items()}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("sweep", "frame", "both", "lifecycle"), default="both")
    ap.add_argument("--deal", choices=("dealt", "undealt"), default="dealt",
                    help="undealt: EPH_CRAFT_SORT=0, knot columns in craft order on both sides (the library reads it once per process)")
    ap.add_argument("--craft", type=int, default=262144)
    ap.add_argument("--knots", type=int, default=364)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5
    if ea.device_count() < 1:
        raise SystemExit("craft_gather_timing.py needs a HIP device: a timing without one says nothing")
    os.environ["EPH_CRAFT_SORT"] = "0" if args.deal == "undealt" else "2"     # before the first batch of the process is created
    result = {"device": ea.device_name(), "library": str(ea.LIB_PATH.name), "reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
              "deal": args.deal, "EPH_CRAFT_SORT": os.environ["EPH_CRAFT_SORT"]}
    if args.case in ("sweep", "both"):
        result["sweep"] = sweep_case(args)
    if args.case in ("frame", "both"):
        result["frame"] = frame_case(args)
    if args.case == "lifecycle":
        result["lifecycle"] = lifecycle_case(args)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
