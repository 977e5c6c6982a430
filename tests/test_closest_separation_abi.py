"""CPU: eph_closest_separation and eph_craft_batch_closest_separation (the app's target search, setup_target_plotting) are part of the
boundary -- declared, exported, bound, wrapped -- and refuse a missing ephemeris / batch before they touch a device. What they
compute is checked on the GPU (test_gpu_closest_separation.py)."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np

from conftest import ROOT

REQUEST_FIELDS = ["int32_t source_body, target_body", "int64_t source_knot_first, source_knot_count",
                  "int64_t target_knot_first, target_knot_count", "double left, right", "double precision", "int64_t max_iterations",
                  "int32_t metric"]
HOST_ARGS = ["const eph_ephemeris *e", "int64_t n_requests", "const eph_separation_request *requests", "int64_t n_knots",
             "const double *knot_t", "const double *knot_pos_xyz", "const double *knot_vel_xyz", "uint8_t *out_found", "double *out_time",
             "double *out_distance", "int32_t *out_iterations", "int32_t *out_status", "double *out_failed_at"]
BATCH_ARGS = ["eph_craft_batch *b", "int64_t n_requests", "const eph_separation_request *requests", "const int64_t *craft",
              "const int64_t *target_craft", "uint8_t *out_found", "double *out_time", "double *out_distance", "int32_t *out_iterations",
              "int32_t *out_status", "double *out_failed_at"]


def test_closest_separation_is_declared_exported_and_bound(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"typedef\s+struct\s+eph_separation_request\s*\{([^}]*)\}\s*eph_separation_request\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_separation_request"
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == REQUEST_FIELDS
    for name, want in (("eph_closest_separation", HOST_ARGS), ("eph_craft_batch_closest_separation", BATCH_ARGS)):
        m = re.search(rf"int32_t\s+{name}\s*\(([^)]*)\)\s*;", code)
        assert m, f"include/ephemeris_amd.h does not declare {name}"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == want
        assert name in product_lib.ABI_SYMBOLS
        assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), name)
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(product_lib.closest_separation) and callable(getattr(product_lib.SpacecraftBatch, "closest_separation"))
    assert C.sizeof(product_lib.SeparationRequest) == 80             # the C layout: 2 x i32, 4 x i64, 3 x f64, i64, i32 + padding
    assert [f[0] for f in product_lib.SeparationRequest._fields_] == [
        "source_body", "target_body", "source_knot_first", "source_knot_count", "target_knot_first", "target_knot_count", "left", "right",
        "precision", "max_iterations", "metric"]
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "closest_separation" in hpp and "eph_craft_batch_closest_separation" in hpp
    assert (ROOT / "examples" / "craft_separation.cpp").exists()


def test_craft_separation_example_compiles_and_links(product_lib, tmp_path):
    """examples/craft_separation.cpp against the product alone, warning-free (the flags of test_craft_plot_abi.py); without a device
    its first compute call throws Error{EPH_ERR_NO_DEVICE} (exit 77)."""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_separation_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_separation.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if product_lib.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and len(lines) == 6 and all("status 0, found 1" in x for x in lines), (r.stdout, r.stderr)


def test_a_null_handle_is_refused_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing ephemeris / batch whatever the other arguments, before any device work (this machine may
    have no device at all), and nothing is written into the caller's buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    dp, u8p, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    R = product_lib.SeparationRequest
    rq = (R * 2)(R(-1, 0, 0, 2, 0, 0, 0.0, 86400.0, 0.001, 1000, 0), R(-1, -1, 0, 2, 2, 2, 0.0, 86400.0, 0.001, 1000, 1))
    batch_rq = (R * 2)(R(-1, 0, 0, 0, 0, 0, 0.0, 86400.0, 0.001, 1000, 0), R(-1, -1, 0, 0, 0, 0, 0.0, 86400.0, 0.001, 1000, 1))
    kt, kp, kv = np.arange(4.0), np.zeros(12), np.zeros(12)
    craft, target = np.array([0, 1], dtype=np.int64), np.array([-1, 0], dtype=np.int64)
    found = np.full(2, 0xA5, np.uint8)
    time, dist, fail = np.full(2, -7.25), np.full(2, -7.25), np.full(2, -7.25)
    it, st = np.full(2, -99, np.int32), np.full(2, -99, np.int32)
    outs = (found.ctypes.data_as(u8p), time.ctypes.data_as(dp), dist.ctypes.data_as(dp), it.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
            fail.ctypes.data_as(dp))
    out_forms = [outs, (None,) * 6] + [outs[:k] + (None,) + outs[k + 1:] for k in range(6)]
    knot_forms = [(4, kt.ctypes.data_as(dp), kp.ctypes.data_as(dp), kv.ctypes.data_as(dp)), (0, None, None, None), (4, None, None, None),
                  (-1, None, None, None)]
    calls = 0
    for (n, requests), knots, o in itertools.product(((2, rq), (1, rq), (0, None), (-1, None), (2, None)), knot_forms, out_forms):
        assert L.eph_closest_separation(None, n, requests, *knots, *o) == bad
        calls += 1
    for (n, requests), cr, tg, o in itertools.product(((2, batch_rq), (2, rq), (1, batch_rq), (0, None), (-1, None), (2, None)),
                                                      (None, craft.ctypes.data_as(i64p)), (None, target.ctypes.data_as(i64p)), out_forms):
        assert L.eph_craft_batch_closest_separation(None, n, requests, cr, tg, *o) == bad
        calls += 1
    assert calls == 5 * 4 * 8 + 6 * 2 * 2 * 8
    assert (found == 0xA5).all() and (time == -7.25).all() and (dist == -7.25).all() and (fail == -7.25).all()
    assert (it == -99).all() and (st == -99).all()
