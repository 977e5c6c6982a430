"""Where a workgroup of k_lm_step_wg<12, 16> is at which shader-clock tick: the s_memtime stamps of a tuning build
(scripts/build_exp.sh NAME -DEPH_EXPERIMENTS=1 -DEPH_WG_STAMPS=1, csrc/step_wg.hip), read with eph_wg_stamps.

    python scripts/step_entry_stamps.py ephemeris_explorer_amd/libephemeris_amd_exp_NAME.so [launches]

4096 bodies, QuinlanTremaine12. After a second of back-to-back steps: `launches` times (default 200) a batch of 20 steps, a
synchronise and the stamps of the batch's last launch (workgroup 7, lane 0 of each of the twelve waves). Printed per wave and stamp:
the median over the launches of (stamp - the earliest entry stamp of that launch), in ticks, and the step time of the run so that
ticks can be set against microseconds. Stamps: 0 entry, 1 first tile data arrived, 2 at barrier B_0, 3 behind B_0, 4 behind the
tile loop, 5 behind the hand-over barrier, 6 end (tail wave)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from ephemeris_explorer_amd.workloads import plummer

lib = C.CDLL(sys.argv[1])
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 200
vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
dp = C.POINTER(C.c_double)
lib.eph_nbody_create.argtypes = [i32, dp, dp, dp, f64, f64, C.c_char_p, C.POINTER(vp)]
lib.eph_nbody_advance.argtypes = [vp, i64]
lib.eph_nbody_sync.argtypes = [vp]
lib.eph_wg_stamps.argtypes = [C.POINTER(C.c_uint64)]
n = 4096
pos, vel, mu = plummer(n)
h = vp()
assert lib.eph_nbody_create(n, pos.ctypes.data_as(dp), vel.ctypes.data_as(dp), mu.ctypes.data_as(dp), 0.0, 1.0 / 1024.0, b"QuinlanTremaine12",
                            C.byref(h)) == 0
lib.eph_nbody_advance(h, 12)
t = time.time()
while time.time() - t < 1.0:
    lib.eph_nbody_advance(h, 500)
    lib.eph_nbody_sync(h)
t = time.time()
lib.eph_nbody_advance(h, 2000)
lib.eph_nbody_sync(h)
us = (time.time() - t) / 2000 * 1e6
rows = np.zeros((launches, 12, 8), dtype=np.uint64)
for k in range(launches):
    lib.eph_nbody_advance(h, 20)
    assert lib.eph_wg_stamps(rows[k].ctypes.data_as(C.POINTER(C.c_uint64))) == 0
rel = rows.astype(np.int64) - rows[:, :, 0].min(axis=1).astype(np.int64)[:, None, None]
med = np.median(rel, axis=0)
role = {0: "one-body", 4: "chain", 8: "tail"}
print(f"{os.path.basename(sys.argv[1])}: {us:.2f} us per step (host clock, 2000 steps); ticks after the workgroup's first entry, median of {launches}")
print("wave role        entry    data  at B_0 past B_0    loop hand-over   end")
for w in range(12):
    name = role.get(w, f"rank {w >> 2} simd {w & 3}")
    cells = ["%7d" % med[w, k] if rows[:, w, k].any() else "      -" for k in range(7)]
    print(f"{w:>4} {name:<12}" + " ".join(cells))
end = rel[:, :, :7].max(axis=(1, 2))
print("last stamp of the workgroup: median %d ticks, min %d, max %d" % (np.median(end), end.min(), end.max()))
