"""CPU: eph_craft_batch_restart (flight-plan restart of a spacecraft batch in place) is part of the boundary -- declared with its exact
argument list, exported, bound, wrapped in Python and C++ -- and refuses a missing batch or bad arguments before it touches a device.
What it computes is checked on the GPU (test_gpu_craft_restart.py)."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT


def test_craft_batch_restart_is_declared_exported_and_bound(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int32_t\s+eph_craft_batch_restart\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_restart"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["eph_craft_batch *b", "const uint8_t *which", "const int64_t *burn_offset", "const double *burn_start",
                    "const double *burn_end", "const double *burn_acc_xyz", "const int32_t *burn_ref", "const double *plan_end",
                    "const eph_adaptive_params *params", "double *restart_epoch", "int32_t *outcome"]
    assert "eph_craft_batch_restart" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_restart")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(getattr(product_lib.SpacecraftBatch, "restart"))
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "restart(" in hpp and "eph_craft_batch_restart" in hpp
    assert (ROOT / "examples" / "craft_restart.cpp").exists()


def test_craft_batch_restart_refuses_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing batch whatever the other arguments, before any device work (this machine may have no
    device at all), and nothing is written into the caller's output buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    dp, i32p, i64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    n = 4
    off = np.array([0, 1, 1, 2, 2], dtype=np.int64)
    bad_off = np.array([0, 2, 1, 2, 2], dtype=np.int64)                # decreasing: not a CSR
    bs, be = np.array([10.0, 20.0]), np.array([11.0, 21.0])
    ba = np.zeros(6)
    br = np.array([-1, 1], dtype=np.int32)
    which = np.array([1, 0, 1, 0], dtype=np.uint8)
    plan_end = np.full(n, 1e9)
    params = product_lib.AdaptiveParams.default(1e-3)
    epoch = np.full(n, -7.25)
    outcome = np.full(n, 0x5A5A, dtype=np.int32)
    ep, op = epoch.ctypes.data_as(dp), outcome.ctypes.data_as(i32p)
    for o in (off, bad_off, None):
        for w in (which, None):
            for pr in (C.byref(params), None):
                for pe in (plan_end.ctypes.data_as(dp), None):
                    args = (None if o is None else o.ctypes.data_as(i64p), bs.ctypes.data_as(dp), be.ctypes.data_as(dp), ba.ctypes.data_as(dp),
                            br.ctypes.data_as(i32p))
                    assert L.eph_craft_batch_restart(None, None if w is None else w.ctypes.data_as(u8p), *args, pe, pr, ep, op) == bad
                    assert L.eph_craft_batch_restart(None, None, *args, pe, pr, None, None) == bad
    assert (epoch == -7.25).all() and (outcome == 0x5A5A).all()
