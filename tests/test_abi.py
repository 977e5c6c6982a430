"""CPU: the C-ABI library builds for gfx950 without a GPU, loads, exports every symbol the header declares, and
fails LOUDLY (no fallback) when there is no device. Host-only entry points are checked against the oracle."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import orc


def header_functions():
    text = (ROOT / "include" / "ephemeris_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eph_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(product_lib):
    names = header_functions()
    assert len(names) >= 40
    lib = ctypes.CDLL(str(product_lib.LIB_PATH))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ephemeris_amd.h but not exported"
    assert sorted(product_lib.ABI_SYMBOLS) == names
    # the COMPLETE dynamic symbol table (functions, kernel handles, data, weak template instantiations -- every class nm knows)
    # is the header's list: csrc/exports.map makes everything else local
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(product_lib.LIB_PATH)]).decode()
    table = [ln.split() for ln in out.splitlines() if ln.strip()]
    exported = {f[-1].split("@")[0] for f in table}
    assert exported == set(names), sorted(exported ^ set(names))[:10]
    assert all(f[-2] == "T" for f in table), [f for f in table if f[-2] != "T"][:5]


def header_prototypes():
    """name -> (return type, [parameter declarations]) for every function include/ephemeris_amd.h declares"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ephemeris_amd.h").read_text(), flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^([\w \t*]+?)\b(eph_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = [" ".join(q.split()) for q in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return protos


def test_ctypes_signatures_match_the_header(product_lib):
    """Every declared function is bound with the header's signature: as many argtypes as parameters, a pointer type wherever the
    header has a pointer, an array or the callback, the exact fixed-width type for every scalar, and the declared kind of return."""
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
               "double": ctypes.c_double}
    protos = header_prototypes()
    assert sorted(protos) == header_functions()
    L = product_lib._lib()
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None, f"{name}: no argtypes"
        assert len(fn.argtypes) == len(params), f"{name}: {len(fn.argtypes)} argtypes for {len(params)} parameters"
        for k, (decl, ct) in enumerate(zip(params, fn.argtypes)):
            if "*" in decl or "[" in decl or decl.split()[0] == "eph_exchange_fn":
                assert ct in (ctypes.c_void_p, ctypes.c_char_p, product_lib.EXCHANGE_FN) or issubclass(ct, ctypes._Pointer), \
                    f"{name} parameter {k} ({decl}): {ct} is not a pointer type"
            else:
                kind = [w for w in decl.split()[:-1] if w != "const"]
                assert len(kind) == 1 and kind[0] in scalars, f"{name} parameter {k} ({decl}): a scalar type this test does not know"
                assert ct is scalars[kind[0]], f"{name} parameter {k} ({decl}): {ct}"
        if ret == "void":
            assert fn.restype is None, name
        elif ret == "const char *":
            assert fn.restype is ctypes.c_char_p, name
        elif ret == "eph_nbody *":
            assert fn.restype is ctypes.c_void_p, name
        else:
            assert ret == "int32_t" and fn.restype in (ctypes.c_int32, ctypes.c_int), (name, ret, fn.restype)


def test_code_object_is_gfx950(product_lib):
    blob = product_lib.LIB_PATH.read_bytes()
    assert b"gfx950" in blob and b"k_lm_step" in blob and b"k_lm_persistent" in blob


def test_status_strings(product_lib):
    L = product_lib._lib()
    assert L.eph_status_string(3) == b"integration bound reached"     # StepError Display, lib.rs:323-331
    assert L.eph_status_string(1) == b"step size underflow"
    assert b"no CPU path" in L.eph_status_string(-2)


def test_coefficient_entry_points_match_oracle(product_lib):
    for name in ("BlanesMoan6B", "BlanesMoan14A", "McLachlanSS17", "Pefrl"):
        A, B, f = product_lib.srkn_coeffs(name)
        Ao, Bo, fo = orc.srkn_coeffs(name)
        assert f == fo and np.array_equal(A, Ao) and np.array_equal(B, Bo)
    for name in ("QuinlanTremaine12", "Stormer13"):
        a, b = product_lib.elm2_coeffs(name), orc.elm2_coeffs(name)
        assert a["order"] == b["order"] and a["inv_beta_d"] == b["inv_beta_d"] and a["inv_cowell_d"] == b["inv_cowell_d"]
        for k in ("w_alpha", "w_beta", "cowell"):
            assert np.array_equal(a[k], b[k])


def test_no_device_fails_loudly(product_lib):
    if product_lib.device_count() > 0:
        pytest.skip("a device is visible here")
    with pytest.raises(product_lib.EphemerisError) as e:
        product_lib.accel_eval(np.zeros((2, 3)), np.ones(2))
    assert e.value.status == product_lib.ERR_NO_DEVICE
    with pytest.raises(product_lib.EphemerisError):
        product_lib.NBodyIntegration(np.zeros((2, 3)), np.zeros((2, 3)), np.ones(2), 0.0, 1.0)
    with pytest.raises(product_lib.EphemerisError):
        product_lib.least_squares_fit(3, np.zeros((1, 9, 3)))


def test_product_never_imports_the_oracle():
    import ephemeris_explorer_amd
    pkg = ROOT / "ephemeris_explorer_amd"
    for p in list(pkg.rglob("*.py")) + list(pkg.rglob("*.cpp")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.h")):
        text = p.read_text()
        assert "import orc" not in text and "eph_oracle" not in text and "pyoracle" not in text, p


def test_header_is_plain_c_and_the_c_example_links(product_lib, tmp_path):
    """include/ephemeris_amd.h is the boundary a cgo / Rust-FFI / C caller binds: it must compile as C99 (pedantic) and as
    C++11, and examples/propagate.c -- the propagator seam driven from plain C -- must build and link against the library.
    Without a device the example stops at its first compute call with EPH_ERR_NO_DEVICE (exit 77): no CPU fallback."""
    import subprocess
    from conftest import ROOT
    hdr = ROOT / "include" / "ephemeris_amd.h"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", str(hdr)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", str(hdr)])
    exe = tmp_path / "propagate"
    libdir = ROOT / "ephemeris_explorer_amd"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "propagate.c"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    import ephemeris_explorer_amd as ea
    if ea.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr.lower() or "-2" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "inside=1" in r.stdout, (r.stdout, r.stderr)
    # examples/craft.c: the spacecraft seam (a batch of one with the app's solout) from plain C
    exe2 = tmp_path / "craft"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "craft.c"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-lm", "-o", str(exe2)])
    r = subprocess.run([str(exe2)], capture_output=True, text=True)
    if ea.device_count() < 1:
        assert r.returncode == 77, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "apsides" in r.stdout, (r.stdout, r.stderr)


def test_cpp_operator_surface_compiles_and_links(product_lib, tmp_path):
    """include/ephemeris_amd.hpp (the reference's trait surface over the C ABI, header-only C++17) compiles warning-free and
    examples/propagate.cpp links against the product alone; without a device its first compute call throws
    Error{EPH_ERR_NO_DEVICE} (exit 77): the wrapper has no CPU path either."""
    import subprocess
    from conftest import ROOT
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "propagate_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "propagate.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    import ephemeris_explorer_amd as ea
    if ea.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "inside=1" in r.stdout, (r.stdout, r.stderr)
    text = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "oracle" not in text and "torch" not in text


def test_debug_hooks_are_not_in_the_product(product_lib):
    """csrc/eph_debug.h: the ten eph_debug_* hooks are exported by the test-hooks library (the product's objects + debug_api.o +
    debug_kernels.o + pair_debug.pv<k>.o, k = 0..6) and by tuning builds, never by libephemeris_amd.so; the product exports the
    header's functions and no other eph_* name, and the per-order hook kernels (csrc/pair_debug.hip) are in no symbol of it."""
    hooks_lib = product_lib.LIB_PATH.with_name("libephemeris_amd_testhooks.so")
    assert hooks_lib.exists(), "ephemeris_explorer_amd.build builds it beside the product"
    text = (ROOT / "ephemeris_explorer_amd" / "csrc" / "eph_debug.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    debug = sorted(set(re.findall(r"\b(eph_debug_[a-z0-9_]+)\s*\(", text)))
    assert len(debug) == 10
    assert not any(n.startswith("eph_debug") for n in header_functions())

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", str(path)]).decode()
        return set(re.findall(r" T (eph_[a-z0-9_]+)", out))
    assert exported(hooks_lib) == set(header_functions()) | set(debug)
    assert not (exported(product_lib.LIB_PATH) & set(debug))
    # -fvisibility=hidden: no C++ function of the implementation is a dynamic symbol of the product either
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(product_lib.LIB_PATH)]).decode()
    leaked = [ln for ln in out.splitlines() if " T " in ln and " T eph_" not in ln and "__device_stub__" not in ln]
    assert not leaked, leaked[:5]
    assert product_lib._lib().eph_abi_version() == 3
    # the full symbol tables (the kernels' host stubs and handles are local symbols, not stripped)
    defined = lambda path: subprocess.check_output(["nm", "--defined-only", str(path)]).decode().split()
    assert not [s for s in defined(product_lib.LIB_PATH) if "k_debug_inv_r3" in s or "k_debug_quot" in s]
    in_hooks = defined(hooks_lib)
    for k in range(7):
        for kernel in ("k_debug_inv_r3", "k_debug_inv_r3_sweep", "k_debug_quot"):
            mangled = f"3pv{k}{len(kernel)}{kernel}E"                   # eph::pv<k>::<kernel>(
            assert any(mangled in s for s in in_hooks), (k, kernel)


def test_every_table_slot_holds_its_own_order(product_lib):
    """slot k of the product's launcher table (csrc/pair_table.hip through dispatch.cpp) and of the hooks' (csrc/pair_debug.hip
    through debug_api.cpp) was compiled for evaluation order k. A host function of the hooks library: no device is touched."""
    import sys
    sys.path.insert(0, str(ROOT / "tests"))
    import hooks
    assert hooks.load().table_variants() == (list(range(7)), list(range(7)))


def test_integration_shims_use_only_declared_names():
    """INTEGRATION.md writes the Rust shims (extern "C" block + trait impls) a maintainer would add; no Rust toolchain exists in the
    image, so they have never been compiled -- what CAN be checked is that every eph_* function the shim text names is one
    include/ephemeris_amd.h declares (missing #3)."""
    text = (ROOT / "INTEGRATION.md").read_text()
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    known = set(re.findall(r"\b(eph_[a-z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    used = set(re.findall(r"\b(eph_[a-z0-9_]+)\b", text))
    prose = {"eph_oracle", "eph_prop_", "eph_craft_batch_", "eph_nbody_", "eph_solution_", "eph_debug", "eph_debug_"}   # file / prefix mentions
    unknown = sorted(n for n in used - known - prose if not n.endswith("_"))
    assert not unknown, f"INTEGRATION.md names functions the header does not declare: {unknown}"
    fns = set(header_functions())
    called = {n for n in used if n in fns}
    assert len(called) >= 50                         # the shims bind most of the boundary (94 - 7 hooks = 87 functions)
    assert "never been compiled" in text or "never met" in text     # section 0 says so in one line


def test_live_ephemeris_entry_points_refuse_null_handles(product_lib):
    """ABI 3's new entry points return EPH_ERR_BAD_ARGUMENT for missing handles before they touch a device (no compute without a GPU)."""
    import ctypes as C
    L = product_lib._lib()
    bad = product_lib.ERR_BAD_ARGUMENT
    f = C.c_int32(7)
    n = C.c_uint64(0)
    h = C.c_void_p()
    assert L.eph_ephemeris_append(None, None, 1) == bad
    assert L.eph_ephemeris_merge(None, None, 1) == bad
    assert L.eph_ephemeris_clear(None, -1, 0.0, 0) == bad
    assert L.eph_ephemeris_info(None, -1, None, None, None, None) == bad
    assert L.eph_ephemeris_is_valid_at(None, 0.0, C.byref(f)) == bad and f.value == 7
    assert L.eph_ephemeris_export(None, None, 0, C.byref(n)) == bad
    assert L.eph_ephemeris_import(None, 0, C.byref(h)) == bad and not h.value
    assert L.eph_ephemeris_import((C.c_char * 8)(), 8, C.byref(h)) == bad and not h.value      # shorter than an image header
    assert L.eph_craft_batch_retry_failed(None) == bad
