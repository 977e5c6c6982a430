"""Wall time of the multistep start-up, for profiles/startup_small.md:

  (a) one fresh 32-body QuinlanTremaine12 handle, advance(12) + sync()                         [us]
  (b) the same on a <Double> handle                                                            [us]
  (c) ensembles of 256 and 1024 fresh 32-body systems, advance_many(12 + 10 000) + sync        [ms]
  (d) k_srkn_small / k_srkn_double_small, which share their stage loop with the start-up kernel: device time per
      BlanesMoan14A step of one launch of 20 000 steps at 32 bodies                            [us]

Handles are created outside the timed region; the first
repetitions are discarded as warm-up; the rest are reported as median, minimum, maximum and quartiles.

    python scripts/time_startup.py [--package-root DIR] [--reps N] [--ensemble-reps N] [--tag NAME]

--package-root: the directory that holds the ephemeris_explorer_amd package to measure (default: this checkout) -- a build of
another commit is measured with the same script, on the same box, in a process of the same layout. One JSON line per figure."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
L, STEADY = 12, 10_000


def spread(xs):
    q = statistics.quantiles(xs, n=4) if len(xs) >= 4 else [min(xs), statistics.median(xs), max(xs)]
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), q1=q[0], q3=q[2], n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=str(ROOT))
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--ensemble-reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--tag", default="this checkout")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd.systems import load_system

    assert Path(ea.__file__).resolve().is_relative_to(Path(args.package_root).resolve()), ea.__file__
    ea.set_device(0)
    s = load_system(ROOT / "tests/golden/systems/full_solar_system_2433282.5")
    assert s.n == 32

    def fresh(compensated=False, scale=1.0):
        return ea.NBodyIntegration(s.pos * scale, s.vel, s.mu, s.epoch, s.dt, "QuinlanTremaine12", compensated=compensated)

    def out(**kw):
        print(json.dumps(dict(tag=args.tag, device=ea.device_name(), **kw)), flush=True)

    for name, compensated in (("a: advance(12) + sync, plain", False), ("b: advance(12) + sync, <Double>", True)):
        us = []
        for r in range(args.warmup + args.reps):
            g = fresh(compensated)
            g.sync()
            t0 = time.perf_counter()
            g.advance(L)
            g.sync()
            dt = time.perf_counter() - t0
            if r >= args.warmup:
                us.append(dt * 1e6)
        out(figure=name, unit="us", **spread(us))

    # the step kernels that share the stage loop with the start-up kernel: device time per step of one launch of 20 000 steps
    for name, compensated in (("d: k_srkn_small, BlanesMoan14A, per step", False), ("d: k_srkn_double_small, BlanesMoan14A, per step", True)):
        g = ea.NBodyIntegration(s.pos, s.vel, s.mu, s.epoch, s.dt, "BlanesMoan14A", compensated=compensated)
        g.advance(200)
        g.enable_timing()
        us = []
        for r in range(2 + 6):
            before = g.kernel_time()[0]
            g.advance(20_000)
            g.sync()
            if r >= 2:
                us.append((g.kernel_time()[0] - before) * 1e3 / 20_000)
        out(figure=name, unit="us (device)", **spread(us))

    for size in (256, 1024):
        ms = []
        for r in range(1 + args.ensemble_reps):
            # distinct systems: member i's positions scaled by (1 + i / 2^20)
            gang = [fresh(scale=1.0 + i / 1048576.0) for i in range(size)]
            for g in gang:
                g.sync()
            t0 = time.perf_counter()
            ea.advance_many(gang, L + STEADY)
            for g in gang:
                g.sync()
            dt = time.perf_counter() - t0
            if r >= 1:
                ms.append(dt * 1e3)
            checks = np.array([g.state()[3] for g in (gang[0], gang[-1])])
            assert (checks == L + STEADY).all(), checks
            del gang
        out(figure=f"c: ensemble of {size}, advance_many({L} + {STEADY}) + sync", unit="ms", **spread(ms))


if __name__ == "__main__":
    main()
