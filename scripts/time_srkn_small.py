#!/usr/bin/env python
"""What the single-workgroup SRKN kernels (csrc/step_srkn_small.hip) cost against the per-stage launches they replace, from one
process and one build -> profiles/srkn_small.md.

  * all eight symplectic tables at 32 (the shipped system), 10 and 3 bodies (its first bodies), plain and `<Double>` handles: the one
    launch (path 0) and the per-stage launches (set_path(1)) on the same handle type, interleaved, after a warm-up advance of each.
    The one launch: device time from eph_nbody_kernel_time (HIP events around the launch) over 20 000 steps, and the wall time of the
    same advance + sync. The per-stage path opens no timing interval, so its figure is the wall time of advance + sync over 2 000
    steps (it is bound by launches: the time per step does not depend on the step count);
  * the wall time of the device's BlanesMoan14A convergence sweep (ephemeris_explorer_amd.convergence) beside the one-core CPU
    oracle's (oracle/orc.py convergence(native=True)) on this host, and the shape of its rows.

    python scripts/time_srkn_small.py [--out profiles/srkn_small.md] [--commit TEXT] [--resources-json FILE] [--no-sweep]
    python scripts/time_srkn_small.py --resources-only --resources-json FILE     (no device: compiles, writes the register figures)

Whatever the output file holds from the heading "## One-line changes" on is written by hand (which test notices which defect) and is
kept as it is.

The kernels' VGPR / LDS figures come from the compiler (-Rpass-analysis=kernel-resource-usage with the build's flags);
--resources-json caches them so that a machine without the time to compile can reuse them."""
import argparse
import json
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

YEAR = 365 * 86400.0
TABLES = ("BlanesMoan6B", "BlanesMoan11B", "BlanesMoan14A", "ForestRuth", "McLachlanO4", "McLachlanSS17", "Pefrl", "Ruth")
SIZES = (32, 10, 3)
STEPS_ONE, STEPS_STAGED, WARM = 20_000, 2_000, 200
HAND_WRITTEN = "## One-line changes"


def kernel_resources(cache=None, sources=("step_srkn_small.hip", "step_small.hip", "step_double_small.hip")):
    if cache and Path(cache).exists():
        return json.loads(Path(cache).read_text())
    from ephemeris_explorer_amd import build as b
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in sources:
            cmd = [b.hipcc(), *b.FLAGS, "-DEPH_PAIR_VARIANT=0", "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
                   str(b.CSRC / src), "-o", str(Path(tmp) / "unit.o")]
            text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
            name = None
            for line in text.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0]
                    out[name] = {}
                m = re.search(r"remark:(?: \S+:\d+:\d+:)?\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
                if m and name:
                    out[name][m.group(1)] = int(m.group(2))
    if cache:
        Path(cache).parent.mkdir(parents=True, exist_ok=True)
        Path(cache).write_text(json.dumps(out, indent=1))
    return out


def timed(g, steps):
    """(device microseconds per step or None where the path opens no timing interval, wall microseconds per step, launches counted)"""
    g.sync()
    ms0, n0 = g.kernel_time()
    t = time.perf_counter()
    g.advance(steps)
    g.sync()
    wall = time.perf_counter() - t
    ms1, n1 = g.kernel_time()
    return ((ms1 - ms0) * 1e3 / steps if n1 > n0 else None), wall * 1e6 / steps, n1 - n0


def measure(ea, pos, vel, mu, t0, h, table, compensated, repeats=3):
    """-> (device us per step of the one launch, its wall us per step, wall us per step of the per-stage launches): medians"""
    one = ea.NBodyIntegration(pos, vel, mu, t0, h, table, compensated=compensated)
    staged = ea.NBodyIntegration(pos, vel, mu, t0, h, table, compensated=compensated)
    staged.set_path(1)
    for g in (one, staged):
        g.enable_timing()
        timed(g, WARM)
    dev, wall, st = [], [], []
    for _ in range(repeats):
        d, w, launches = timed(one, STEPS_ONE)
        assert launches == 1 and d is not None, (table, compensated, launches)
        dev.append(d)
        wall.append(w)
        st.append(timed(staged, STEPS_STAGED)[1])
    return statistics.median(dev), statistics.median(wall), statistics.median(st)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "srkn_small.md"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--resources-json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    res = kernel_resources(a.resources_json)
    if a.resources_only:
        print(json.dumps(res, indent=1))
        return 0

    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd.systems import load_system
    from ephemeris_explorer_amd.workloads import profile_stamp
    from oracle import orc
    if ea.device_count() < 1:
        print("no HIP device: nothing is measured without one", file=sys.stderr)
        return 77
    s = load_system(ROOT / "tests" / "golden" / "systems" / "full_solar_system_2433282.5")
    tables = {t: ea.srkn_coeffs(t) for t in TABLES}
    commit = a.commit or profile_stamp("nbody")["profile_commit"] or "unknown"
    lines = ["# The single-workgroup SRKN kernels: one launch against one launch per stage", "",
             f"Written by `scripts/time_srkn_small.py` (one process, one build). Commit: {commit}. Device: {ea.device_name()}.",
             f"The first n bodies of the shipped system, h = 600 s. One launch: `eph_nbody_kernel_time` (HIP events around the launch) over {STEPS_ONE}",
             f"steps, and the wall time of the same `advance` + `sync`. Per-stage launches (`set_path(1)`): wall time of `advance` + `sync` over",
             f"{STEPS_STAGED} steps (that path opens no timing interval). Medians of three interleaved repeats after a warm-up advance of each.", "",
             "| bodies | table (stages, FSAL) | state | one launch, us/step (device) | us/evaluation | one launch, us/step (wall) | per-stage, us/step (wall) | per-stage / one launch (wall) |",
             "|---|---|---|---|---|---|---|---|"]
    slower = []
    for n in SIZES:
        for table in TABLES:
            stages, fsal = len(tables[table][0]), bool(tables[table][2])
            for compensated in (False, True):
                dev, wall, st = measure(ea, s.pos[:n], s.vel[:n], s.mu[:n], s.epoch, 600.0, table, compensated)
                evals = stages - 1 if fsal else stages
                lines.append(f"| {n} | {table} ({stages}, {'FSAL' if fsal else 'no'}) | {'`<Double>`' if compensated else 'plain'} | {dev:.3f} | "
                             f"{dev / evals:.3f} | {wall:.3f} | {st:.2f} | {st / wall:.1f} |")
                print(lines[-1], flush=True)
                if not wall < st:
                    slower.append((n, table, compensated))
    lines += ["", "Dispatch condition (the one launch is faster per step than the per-stage launches at every measured size and table): " +
              ("holds." if not slower else "DOES NOT HOLD for " + ", ".join(f"{n} bodies {t}{'<Double>' if c else ''}" for n, t, c in slower) + ".")]

    if not a.no_sweep:
        t = time.perf_counter()
        h_dev, rows_dev = ea.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, "BlanesMoan14A", 75.0)   # (ends in get_state: synchronised)
        wall_dev = time.perf_counter() - t
        orc.lib(native=True)                               # built and loaded outside the window
        t = time.perf_counter()
        h_cpu, rows_cpu = orc.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, "BlanesMoan14A", 75.0, native=True)
        wall_cpu = time.perf_counter() - t
        sweep_steps = int(YEAR / 37.5 + sum(YEAR / r[0] for r in rows_dev))
        import numpy as np
        shape = (np.array_equal(rows_dev[:, 0], 75.0 * 2.0 ** np.arange(len(rows_dev))) and bool((rows_dev[:-1, 1] <= 10.0).all())
                 and bool((rows_dev[:-1, 2] <= 1.0).all()) and (rows_dev[-1, 1] > 10.0 or rows_dev[-1, 2] > 1.0) and rows_dev[-1, 0] == 2.0 * h_dev)
        lines += ["", "## The reference's third known answer: the convergence sweep of BlanesMoan14A, 32 bodies, 365 days", "",
                  "| where | answer | rows | wall time |", "|---|---|---|---|",
                  f"| device, `ephemeris_explorer_amd.convergence` ({sweep_steps} steps in all, one launch per run) | {h_dev:.0f} s | {len(rows_dev)} | {wall_dev:.2f} s |",
                  f"| one CPU core of this host, `orc.convergence(native=True)` | {h_cpu:.0f} s | {len(rows_cpu)} | {wall_cpu:.2f} s |", "",
                  f"Rows `75 * 2^k`, every row but the last inside 10 m / 1 m/s, the last at {rows_dev[-1, 0]:.0f} s (the shape tests/test_convergence_pin.py asserts): "
                  + ("yes" if shape else "NO") + ". The answer is 600 s: " + ("yes" if h_dev == 600.0 else "NO") + ".",
                  "The rows agree with the oracle's bit for bit: " + ("yes" if rows_dev.tobytes() == rows_cpu.tobytes() else "NO") + "."]
    lines += ["", "## Kernel resources (compiler, `-Rpass-analysis=kernel-resource-usage`, evaluation order 0)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for name, r in sorted(res.items()):
        if "k_srkn" in name or "k_lm_double_small<12>" in name or "k_lm_small<12, false, false>" in name:
            lines.append(f"| `{name.split('::')[-1]}` | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('ScratchSize [bytes/lane]')} | "
                         f"{r.get('VGPRs Spill')} | {r.get('LDS Size [bytes/block]')} | {r.get('Occupancy [waves/SIMD]')} |")
    out = Path(a.out)
    kept = out.read_text() if out.exists() else ""
    kept = kept[kept.index(HAND_WRITTEN):] if HAND_WRITTEN in kept else ""
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n" + ("\n" + kept if kept else ""))
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
