"""CPU: eph_craft_batch_eval (the batch-wide trajectory evaluation of a spacecraft batch) is part of the boundary -- declared, exported,
bound -- and refuses a missing batch before it touches a device. What it computes is checked on the GPU (test_gpu_craft_eval.py)."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT


def test_craft_batch_eval_is_declared_exported_and_bound(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int32_t\s+eph_craft_batch_eval\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_eval"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["eph_craft_batch *b", "int64_t m", "const double *at", "int32_t per_craft", "int32_t reference_body",
                    "double *out_y", "uint8_t *inside"]
    assert "eph_craft_batch_eval" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_eval")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(getattr(product_lib.SpacecraftBatch, "eval"))
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "state_vectors_at" in hpp and "eph_craft_batch_eval" in hpp
    assert (ROOT / "examples" / "craft_eval.cpp").exists()


def test_craft_batch_eval_refuses_a_null_batch_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing batch whatever the other arguments, before any device work (this machine may have no
    device at all), and nothing is written into the caller's buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    at = np.array([1.0, 2.0, 3.0])
    poison = np.float64(-7.25)
    out = np.full(3 * 6 * 4, poison)
    inside = np.full(3 * 4, 0xA5, dtype=np.uint8)
    cases = [(3, at.ctypes.data_as(dp), 0, -1), (3, at.ctypes.data_as(dp), 1, 0), (0, None, 0, -1), (-1, None, 2, -5),
             (3, None, 0, 10 ** 6), (1, at.ctypes.data_as(dp), 0, 0)]
    for m, atp, per_craft, body in cases:
        for o, i in ((out.ctypes.data_as(dp), inside.ctypes.data_as(u8p)), (out.ctypes.data_as(dp), None), (None, None)):
            assert L.eph_craft_batch_eval(None, m, atp, per_craft, body, o, i) == bad
    assert (out == poison).all() and (inside == 0xA5).all()
