"""CPU: eph_craft_batch_plot_points (the adaptive plot sampler on a spacecraft batch's own knot slabs) is part of the boundary --
declared, exported, bound, wrapped -- and refuses a missing batch before it touches a device. What it computes is checked on the GPU
(test_gpu_craft_plot.py)."""
import ctypes as C
import re
import subprocess

import numpy as np

from conftest import ROOT


def test_craft_batch_plot_points_is_declared_exported_and_bound(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int32_t\s+eph_craft_batch_plot_points\s*\(([^)]*)\)\s*;", code)
    assert m, "include/ephemeris_amd.h does not declare eph_craft_batch_plot_points"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["eph_craft_batch *b", "const eph_plot_view *view", "int64_t n_plots", "const eph_plot_request *requests",
                    "const int64_t *craft", "int64_t capacity", "double *out_t", "float *out_xyz", "int64_t *out_count",
                    "int32_t *out_status", "double *out_failed_at"]
    assert "eph_craft_batch_plot_points" in product_lib.ABI_SYMBOLS
    assert hasattr(C.CDLL(str(product_lib.LIB_PATH)), "eph_craft_batch_plot_points")
    assert product_lib._lib().eph_abi_version() == 3                 # additive: no version bump
    assert callable(getattr(product_lib.SpacecraftBatch, "plot_points"))
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "plot_points" in hpp and "eph_craft_batch_plot_points" in hpp
    assert (ROOT / "examples" / "craft_plot.cpp").exists()


def test_craft_plot_example_compiles_and_links(product_lib, tmp_path):
    """examples/craft_plot.cpp against the product alone, warning-free (the flags of test_cpp_operator_surface_compiles_and_links);
    without a device its first compute call throws Error{EPH_ERR_NO_DEVICE} (exit 77)."""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "craft_plot_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft_plot.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if product_lib.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and len(lines) == 12 and all("status 0" in x for x in lines), (r.stdout, r.stderr)


def test_craft_batch_plot_points_refuses_a_null_batch_without_a_device(product_lib):
    """EPH_ERR_BAD_ARGUMENT for a missing batch whatever the other arguments, before any device work (this machine may have no
    device at all), and nothing is written into the caller's buffers."""
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    dp, fp, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    v = product_lib.PlotView()
    v.camera_position[:] = [1.0e8, 2.0e8, 3.0e8]
    v.grid_matrix3[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    rq = (product_lib.PlotRequest * 2)(product_lib.PlotRequest(-1, -1, 0, 0, 0.0, 86400.0, 0, 1, 1e-4, 8),
                                       product_lib.PlotRequest(-1, 0, 0, 0, 0.0, 86400.0, 1, 1, 1e-4, 8))
    craft = np.array([0, 1], dtype=np.int64)
    ot, ox = np.full(2 * 8, -7.25), np.full(2 * 8 * 3, -7.25, dtype=np.float32)
    cnt, st, fail = np.full(2, -99, np.int64), np.full(2, -99, np.int32), np.full(2, -7.25)
    outs = (ot.ctypes.data_as(dp), ox.ctypes.data_as(fp), cnt.ctypes.data_as(i64p), st.ctypes.data_as(i32p), fail.ctypes.data_as(dp))
    for view in (C.byref(v), None):
        for n_plots, requests in ((2, rq), (1, rq), (0, None), (-1, None), (2, None)):
            for cr in (None, craft.ctypes.data_as(i64p)):
                for capacity in (8, 0, -1):
                    for o in (outs, (None, None) + outs[2:], (None,) * 5):
                        assert L.eph_craft_batch_plot_points(None, view, n_plots, requests, cr, capacity, *o) == bad
    assert (ot == -7.25).all() and (ox == np.float32(-7.25)).all() and (cnt == -99).all() and (st == -99).all() and (fail == -7.25).all()
