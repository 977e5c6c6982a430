"""What the cost-balanced partition of the spacecraft sweep (parallel.balanced_partition) buys, measured on one device without a
second one: a craft's integrator attempts do not depend on the batch it runs in, so ONE sweep of all the craft in one batch gives
the per-craft attempts, and the per-rank sums under any partition follow exactly.

    python scripts/craft_partition.py [--craft N] [--craft-days D] [--population mixed|transfer]
                                      [--population-order blocked|interleaved] [--out FILE.json]

Prints, for world = 2, 4 and 8, the max / mean over ranks of the per-rank attempts under the contiguous split (parallel.shard_range)
and under the balanced one (the snake deal of parallel.craft_cost_estimate, and of the measured attempts themselves: what a caller
that sweeps repeatedly can pass), and the seconds the estimate and the partition take on the host."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import ephemeris_explorer_amd as ea                                   # noqa: E402
from ephemeris_explorer_amd import parallel                            # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system      # noqa: E402
from ephemeris_explorer_amd.workloads import craft_population          # noqa: E402

DAY = 86400.0


def ratio(attempts, blocks):
    per_rank = np.array([attempts[b].sum(dtype=np.int64) for b in blocks], dtype=np.float64)
    return float(per_rank.max() / per_rank.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--craft", type=int, default=65536)
    ap.add_argument("--craft-days", type=float, default=5.0)
    ap.add_argument("--population", default="mixed", choices=["mixed", "transfer"])
    ap.add_argument("--population-order", default="blocked", choices=["blocked", "interleaved"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ea.device_count() < 1:
        raise SystemExit("craft_partition.py needs a HIP device: the attempts come from the device's sweep")
    sysdir = ROOT / "tests/golden/systems/full_solar_system_2433282.5"
    s = load_system(sysdir)
    ship = load_ship(sysdir / "ships" / "Mars Transfer Ship.json")
    sol = ea.NBodyPropagator.from_system(s).propagate(s.epoch + (args.craft_days + 40.0) * DAY)
    eph = ea.Ephemeris(sol, s.mu)
    n = args.craft
    pos, vel, family = craft_population(args.population, n, s, ship, order=args.population_order)
    max_knots = int((1200 if args.population == "transfer" else 400) * args.craft_days) + 64
    batch = ea.SpacecraftBatch(eph, ship.start, pos, vel, "Verner87", max_knots=max_knots)
    tick = time.perf_counter()
    batch.propagate(ship.start + args.craft_days * DAY)
    rec = batch.summary()
    sweep_s = time.perf_counter() - tick
    assert (rec["status"] == 0).all(), np.unique(rec["status"])
    attempts = rec["attempts"].astype(np.int64)
    body_pos, body_vel = parallel.body_states_at(sol, ship.start)
    tick = time.perf_counter()
    cost = parallel.craft_cost_estimate(s.mu, body_pos, body_vel, pos, vel, args.craft_days * DAY)
    estimate_s = time.perf_counter() - tick
    result = {"craft": n, "days": args.craft_days, "population": args.population, "order": args.population_order,
              "device": ea.device_name(), "sweep_s_one_batch": sweep_s, "kernel_ms": batch.kernel_ms(), "attempts": int(attempts.sum()),
              "mean_attempts_per_family": {int(f): float(attempts[family == f].mean()) for f in np.unique(family)},
              "log_correlation": float(np.corrcoef(np.log(cost), np.log(attempts))[0, 1]), "estimate_s": estimate_s, "worlds": {}}
    print(f"{n} craft ({args.population}, {args.population_order}) x {args.craft_days} d on {result['device']}: one batch "
          f"{sweep_s * 1e3:.1f} ms (kernel {result['kernel_ms']:.1f} ms), {result['attempts']} attempts; per family "
          f"{ {k: round(v, 1) for k, v in result['mean_attempts_per_family'].items()} }")
    print(f"estimate {estimate_s * 1e3:.2f} ms on the host (all craft; a rank estimates 1 / world of them), correlation of "
          f"log(estimate) with log(attempts) {result['log_correlation']:.4f}")
    print("world | contiguous | balanced (estimate) | balanced (measured attempts) | partition s")
    for world in (2, 4, 8):
        tick = time.perf_counter()
        blocks = parallel.balanced_partition(cost, world)
        partition_s = time.perf_counter() - tick
        row = {"contiguous": ratio(attempts, [np.arange(*parallel.shard_range(n, r, world)) for r in range(world)]),
               "balanced": ratio(attempts, blocks), "balanced_by_attempts": ratio(attempts, parallel.balanced_partition(attempts, world)),
               "partition_s": partition_s, "block_sizes": [len(b) for b in blocks]}
        result["worlds"][world] = row
        print(f"{world} | {row['contiguous']:.4f} | {row['balanced']:.4f} | {row['balanced_by_attempts']:.4f} | {partition_s:.4f}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
