#!/usr/bin/env python
"""What the SRKN gang (k_srkn_small_many, csrc/step_srkn_small.hip) buys: the figures of profiles/srkn_gang.md. One process measures one
checkout -- this one, or with --root the built checkout of another commit (the parent's) -- and prints one JSON line per figure; the
note is written from the lines of both.

  sweep      the reference's BlanesMoan14A convergence sweep on the shipped 32-body system, one year, h0 = 75 s: wall time of
             ephemeris_explorer_amd.convergence (one run after the other) and, where the checkout has it, of convergence_gang (the
             truth run and five candidates in one advance_many). Both end in a read-back: synchronised.
  ensembles  256 and 1024 fresh copies of that system (each displaced a little, so that no two are one system), BlanesMoan6B and
             BlanesMoan14A, plain and `<Double>`: wall time of advance_many(10 000) + sync of every handle, after a warm-up call of 10
             steps. On a checkout without the gang that call advances every member on its own, one by one: the parent's figure.
  single     one such system, advance(10 000) on its own under enable_timing(): the single-system kernels, device time per evaluation.

    python scripts/time_srkn_gang.py [--root DIR] [--what sweep,ensembles,single] [--repeats 5] [--out FILE]

Wall times are time.perf_counter around synchronised calls; every figure is (median, min, max) over the repeats. Run nothing else on
the device."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

YEAR = 365 * 86400.0
STEPS, WARM = 10_000, 10
TABLES = {"BlanesMoan6B": 6, "BlanesMoan14A": 14}          # force evaluations per step behind the first (FSAL)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), repeats=len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--what", default="sweep,ensembles,single")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = Path(a.root).resolve()
    sys.path.insert(0, str(root))
    import numpy as np
    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd.systems import load_system
    if ea.device_count() < 1:
        print("no HIP device: nothing is measured without one", file=sys.stderr)
        return 77
    assert Path(ea.__file__).resolve().parent.parent == root, ea.__file__
    s = load_system(root / "tests" / "golden" / "systems" / "full_solar_system_2433282.5")
    has_gang = hasattr(ea, "convergence_gang")
    out = open(a.out, "a") if a.out else None

    def emit(**rec):
        rec.update(root=root.name, gang=has_gang, device=ea.device_name())
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    what = a.what.split(",")
    if "single" in what:
        for table, evals in TABLES.items():
            for compensated in (False, True):
                g = ea.NBodyIntegration(s.pos, s.vel, s.mu, s.epoch, 600.0, table, compensated=compensated)
                g.enable_timing()
                g.advance(WARM)
                g.sync()
                us = []
                for _ in range(a.repeats):
                    ms0, _ = g.kernel_time()
                    g.advance(STEPS)
                    g.sync()
                    us.append((g.kernel_time()[0] - ms0) * 1e3 / (STEPS * evals))
                emit(what="single", table=table, compensated=compensated, us_per_evaluation=spread(us))
    if "ensembles" in what:
        rng = np.random.default_rng(7)
        for count in [int(x) for x in a.sizes.split(",")]:
            shift = rng.normal(size=(count, 1, 3)) * 1e-3                     # km: distinct systems, the same cost
            for table, evals in TABLES.items():
                for compensated in (False, True):
                    gang = [ea.NBodyIntegration(s.pos + shift[j], s.vel, s.mu, s.epoch, 600.0, table, compensated=compensated)
                            for j in range(count)]
                    ea.advance_many(gang, WARM)
                    for g in gang:
                        g.sync()
                    wall = []
                    for _ in range(a.repeats):
                        t = time.perf_counter()
                        ea.advance_many(gang, STEPS)
                        for g in gang:
                            g.sync()
                        wall.append(time.perf_counter() - t)
                    per = [w * 1e6 / (STEPS * evals) for w in wall]            # the whole ensemble's wall time per evaluation round
                    emit(what="ensemble", count=count, table=table, compensated=compensated, wall_s=spread(wall),
                         us_per_evaluation_of_all=spread(per), us_per_evaluation_per_system=spread([p / count for p in per]),
                         body_steps_per_s=spread([count * 32 * STEPS / w for w in wall]))
                    del gang
    if "sweep" in what:
        args = (s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, "BlanesMoan14A", 75.0)
        routes = [("convergence", ea.convergence)] + ([("convergence_gang", ea.convergence_gang)] if has_gang else [])
        ea.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + 86400.0, "BlanesMoan14A", 75.0)      # warm-up: one day
        results = {}
        for name, f in routes:
            wall = []
            for _ in range(max(2, a.repeats // 2)):
                t = time.perf_counter()
                h, rows = f(*args)
                wall.append(time.perf_counter() - t)
            results[name] = (h, rows)
            emit(what="sweep", route=name, answer=h, rows=len(rows), wall_s=spread(wall))
        if has_gang:
            emit(what="sweep-agree", same=bool(results["convergence"][0] == results["convergence_gang"][0] and
                                               results["convergence"][1].tobytes() == results["convergence_gang"][1].tobytes()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
