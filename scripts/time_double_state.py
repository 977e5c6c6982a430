#!/usr/bin/env python
"""What the compensated state ("<M><Double>", csrc/double_state.h) costs, from one process and one build -> profiles/double_state.md.

  * 32 bodies (the shipped system), QuinlanTremaine12, 100 000 steady steps per launch: plain and compensated handles interleaved,
    three repeats each, device time from eph_nbody_kernel_time (HIP events around the launch), median and spread;
  * 4096 bodies (Plummer), 200 steady steps of the per-step path, the same way;
  * the wall time of the device's QuinlanTremaine12 convergence sweep (ephemeris_explorer_amd.convergence) beside the one-core CPU
    oracle's (oracle/orc.py convergence(native=True)) on this host.

    python scripts/time_double_state.py [--out profiles/double_state.md] [--commit TEXT] [--resources-json FILE]
    python scripts/time_double_state.py --resources-only --resources-json FILE     (no device: compiles, writes the register figures)

The kernel's VGPR / LDS figures come from the compiler (-Rpass-analysis=kernel-resource-usage on step_double_small.hip with the
build's flags); --resources-json caches them so that a machine without the time to compile can reuse them."""
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


def kernel_resources(cache=None):
    if cache and Path(cache).exists():
        return json.loads(Path(cache).read_text())
    from ephemeris_explorer_amd import build as b
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("step_double_small.hip", "step_small.hip"):
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
    """device milliseconds and launches of one advance(steps) on a started handle"""
    ms0, n0 = g.kernel_time()
    g.advance(steps)
    g.sync()
    ms1, n1 = g.kernel_time()
    return ms1 - ms0, n1 - n0


def compare(ea, pos, vel, mu, t0, h, steps, warm, repeats=3):
    """plain and compensated handles, interleaved -> {kind: (us per step of every repeat, launches per advance)}"""
    hs = {"plain": ea.NBodyIntegration(pos, vel, mu, t0, h), "compensated": ea.NBodyIntegration(pos, vel, mu, t0, h, compensated=True)}
    for g in hs.values():
        g.enable_timing()
        g.advance(12)                                  # the start-up
        timed(g, warm)                                 # first launch of every kernel the window uses
    res = {k: ([], None) for k in hs}
    for _ in range(repeats):
        for k, g in hs.items():
            ms, launches = timed(g, steps)
            res[k][0].append(ms * 1e3 / steps)
            res[k] = (res[k][0], launches)
    return res


def row(label, us, launches):
    return f"| {label} | {statistics.median(us):.3f} | {min(us):.3f} - {max(us):.3f} | {launches} |"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "double_state.md"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--resources-json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    res = kernel_resources(a.resources_json)
    if a.resources_only:
        print(json.dumps(res, indent=1))
        return 0

    import ephemeris_explorer_amd as ea
    from ephemeris_explorer_amd.systems import load_system
    from ephemeris_explorer_amd.workloads import plummer, profile_stamp
    from oracle import orc
    if ea.device_count() < 1:
        print("no HIP device: nothing is measured without one", file=sys.stderr)
        return 77
    s = load_system(ROOT / "tests" / "golden" / "systems" / "full_solar_system_2433282.5")
    small = compare(ea, s.pos, s.vel, s.mu, s.epoch, 600.0, 100_000, 20_000)
    pos, vel, mu = plummer(4096)
    large = compare(ea, pos, vel, mu, 0.0, 1.0 / 1024.0, 200, 50)

    t = time.perf_counter()
    h_dev, rows_dev = ea.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, "QuinlanTremaine12", 75.0)   # (ends in get_state: synchronised)
    wall_dev = time.perf_counter() - t
    orc.lib(native=True)                               # built and loaded outside the window
    t = time.perf_counter()
    h_cpu, rows_cpu = orc.convergence(s.pos, s.vel, s.mu, s.epoch, s.epoch + YEAR, "QuinlanTremaine12", 75.0, native=True)
    wall_cpu = time.perf_counter() - t
    sweep_steps = int(YEAR / 37.5 + sum(YEAR / r[0] for r in rows_dev))

    commit = a.commit or profile_stamp("nbody")["profile_commit"] or "unknown"
    lines = ["# The compensated state `<Double>`: what it costs", "",
             f"Written by `scripts/time_double_state.py` (one process, one build). Commit: {commit}. Device: {ea.device_name()}.",
             "Device time is `eph_nbody_kernel_time` (HIP events around the launches of an advance), plain and compensated handles",
             "interleaved, three repeats each after a warm-up advance of every kernel the window uses; QuinlanTremaine12.", "",
             "| handle | us per step, median | min - max | launches per advance |", "|---|---|---|---|"]
    for k in ("plain", "compensated"):
        lines.append(row(f"32 bodies (shipped system, h = 600 s), 100 000 steps, {k}", *small[k]))
    for k in ("plain", "compensated"):
        lines.append(row(f"4096 bodies (Plummer, h = 1/1024), 200 steps, {k}", *large[k]))
    r32 = statistics.median(small["compensated"][0]) / statistics.median(small["plain"][0])
    r4k = statistics.median(large["compensated"][0]) / statistics.median(large["plain"][0])
    lines += ["", f"Compensated / plain: {r32:.2f} x at 32 bodies (single-workgroup kernels), {r4k:.2f} x at 4096 (per-step launches: the force-only",
              "launch plus one element-wise launch against the plain handle's one fused launch).", "",
              "## The reference's convergence sweep, QuinlanTremaine12, 32 bodies, 365 days", "",
              "| where | answer | rows | wall time |", "|---|---|---|---|",
              f"| device, `ephemeris_explorer_amd.convergence` ({sweep_steps} steps in all) | {h_dev:.0f} s | {len(rows_dev)} | {wall_dev:.2f} s |",
              f"| one CPU core of this host, `orc.convergence(native=True)` | {h_cpu:.0f} s | {len(rows_cpu)} | {wall_cpu:.2f} s |", "",
              f"Device / oracle: {wall_dev / wall_cpu:.2f} (expected below 1: " + ("it is" if wall_dev < wall_cpu else "IT IS NOT -- see DESIGN.md section 9") + ").",
              "The rows agree bit for bit: " + ("yes" if rows_dev.tobytes() == rows_cpu.tobytes() else "NO") + ".", "",
              "## Kernel resources (compiler, `-Rpass-analysis=kernel-resource-usage`, evaluation order 0)", "",
              "| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for name, r in sorted(res.items()):
        if "k_lm_double_small" in name or "k_lm_small<12, false, false>" in name or "k_lm_small<13, false, false>" in name:
            lines.append(f"| `{name.split('::')[-1]}` | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('ScratchSize [bytes/lane]')} | "
                         f"{r.get('VGPRs Spill')} | {r.get('LDS Size [bytes/block]')} | {r.get('Occupancy [waves/SIMD]')} |")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
