"""CPU: eph_craft_batch_gather (a new spacecraft batch out of chosen craft of existing ones) is part of the boundary -- declared with its
exact argument list, exported, bound, wrapped in Python and C++, exemplified -- and refuses bad arguments before it touches a device.
What it computes is checked on the GPU (test_gpu_craft_gather.py), its host plan in test_gather_plan.py."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT


def test_craft_batch_gather_is_declared_exported_and_bound(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int32_t\s+eph_craft_batch_gather\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_gather"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["int32_t n_sources", "eph_craft_batch *const *sources", "int64_t n_out", "const int32_t *source_of",
                    "const int64_t *craft_of", "eph_craft_batch **out"]
    assert "eph_craft_batch_gather" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_gather")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    for name in ("gather", "select", "concat"):
        assert callable(getattr(product_lib.SpacecraftBatch, name)), name
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "eph_craft_batch_gather" in hpp
    for name in ("gather(", "select(", "concat("):
        assert name in hpp, name
    assert (ROOT / "examples" / "craft_fleet.cpp").exists()
    assert len(product_lib.ABI_SYMBOLS) == 103


def test_craft_batch_gather_refuses_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT and *out == NULL for a NULL source array, n_sources <= 0, a NULL source, a NULL out, n_out < 0 and the
    forbidden NULL combinations: all refused before any device work (this machine may have no device at all). The source handles of
    the cases that get as far as looking at one are NULL: nothing is dereferenced."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    source_of = np.zeros(4, dtype=np.int32)
    craft_of = np.arange(4, dtype=np.int64)
    so, co = source_of.ctypes.data_as(i32p), craft_of.ctypes.data_as(i64p)
    null_sources = (C.c_void_p * 2)(None, None)
    poison = 0x5A5A5A5A

    def refused(n_sources, sources, n_out, s, c, text):
        out = C.c_void_p(poison)
        assert L.eph_craft_batch_gather(n_sources, sources, n_out, s, c, C.byref(out)) == bad, text
        assert out.value is None, text                                # *out = NULL
        assert text in L.eph_last_error().decode(), (text, L.eph_last_error().decode())

    refused(1, None, 4, None, co, "sources is NULL")
    refused(0, null_sources, 4, None, co, "n_sources < 1")
    refused(-3, null_sources, 4, so, co, "n_sources < 1")
    refused(2, null_sources, 4, so, co, "source 0 is NULL")
    assert L.eph_craft_batch_gather(1, null_sources, 4, None, co, None) == bad              # a NULL out
    assert "out is NULL" in L.eph_last_error().decode()
    # the rules on the shape of the arguments are decided before any source is looked at
    refused(1, null_sources, -1, None, co, "n_out < 0")
    refused(2, null_sources, -1, so, co, "n_out < 0")
    refused(2, null_sources, 4, None, co, "source_of == NULL needs n_sources == 1")
    refused(1, null_sources, 4, so, None, "craft_of == NULL needs source_of == NULL")
    refused(2, null_sources, 4, so, None, "craft_of == NULL needs source_of == NULL")
    assert (source_of == 0).all() and (craft_of == np.arange(4)).all()
