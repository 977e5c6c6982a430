"""Host wall time of eph_ephemeris_merge in the app's pattern (tests/test_gpu_live_ephemeris.py::test_live_many_small_appends): the
bodies advance two steps at a time, every take_solution is merged into the live table (60 merges) and a small batch chases the
table's end between merges. Only the merge call itself is timed. EPH_AMD_LIBRARY selects the build (profiles/live_table_commit.md
alternates the parent's library and this tree's). Prints one JSON line: the 60 times in microseconds, their median, the revision
before and after, and how many of the merges laid the table out afresh -- replayed from eph_ephemeris_info before and after every
merge with the layout rule of csrc/table_layout.h (room = max(npoly, 32) behind every body), since no build counts them itself."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ephemeris_explorer_amd as ea  # noqa: E402
from ephemeris_explorer_amd.systems import load_ship, load_system  # noqa: E402

DAY = 86400.0


def main():
    golden = ROOT / "tests" / "golden" / "systems"
    s = load_system(golden / "simple_solar_system_2433282.5")
    ship = load_ship(golden / "full_solar_system_2433282.5" / "ships" / "Mars Transfer Ship.json")
    count = np.minimum(s.count, 2)
    g = ea.NBodyPropagator(s.pos, s.vel, s.mu, s.epoch, s.dt, 1, count, s.degree)
    g.step_to(s.epoch + 4.5 * DAY)
    eph = ea.Ephemeris(g.take_solution(), s.mu)
    batch = ea.SpacecraftBatch(eph, ship.start, [ship.pos, ship.pos + 30.0], [ship.vel, ship.vel], "DormandPrince54", max_knots=24576)
    end = s.epoch + 40 * DAY
    info = lambda: [eph.info(b) for b in range(s.n)]                       # noqa: E731
    npoly = [i[2] for i in info()]
    room = [max(n, 32) for n in npoly]                                     # rows left behind every body's polynomials
    rev0, relayouts, us = eph.revision, 0, []
    for _ in range(60):
        g.step_n(2)
        piece = g.take_solution()
        before = info()
        t0 = time.perf_counter()
        eph.merge(piece)
        us.append((time.perf_counter() - t0) * 1e6)
        after = info()
        added = [a[2] - b[2] for a, b in zip(after, before)]
        assert all(a[0] == b[0] and d >= 0 for a, b, d in zip(after, before, added)), "the scenario only appends"
        if any(d > r for d, r in zip(added, room)):
            relayouts += 1
            room = [max(a[2], 32) for a in after]
        else:
            room = [r - d for r, d in zip(room, added)]
        batch.retry_failed().propagate(end)
    print(json.dumps({"library": str(ea.LIB_PATH.name), "merges": len(us), "median_us": float(np.median(us)), "min_us": min(us), "max_us": max(us),
                      "revision_before": rev0, "revision_after": eph.revision, "relayouts": relayouts,
                      "npoly_after": [i[2] for i in info()], "us": [round(x, 1) for x in us]}))


if __name__ == "__main__":
    main()
