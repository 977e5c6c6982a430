"""CPU: the compensated integrator state ("<M><Double>", csrc/double_state.h) is part of the boundary without a new export --
documented in the header, switched on in the Python and C++ wrappers, exemplified -- and the name parser behind it accepts exactly
the suffix. What a tagged handle computes is checked on the GPU (test_gpu_double_state.py)."""
import inspect
import re
import subprocess

from conftest import ROOT, SYSTEMS


def test_the_header_documents_the_double_suffix(product_lib):
    header = (ROOT / "include" / "ephemeris_amd.h").read_text()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct eph_nbody eph_nbody;", header, flags=re.S)
    assert m, "the comment in front of eph_nbody_create"
    text = " ".join(m.group(1).split())
    for needle in ("<Double>", "Double<DVec3>", "QuinlanTremaine12<Double>", "EPH_ERR_BAD_ARGUMENT", "value parts",
                   "not readable through the ABI", "EPH_ERR_UNSUPPORTED"):
        assert needle in text, needle
    assert product_lib._lib().eph_abi_version() == 3                 # no export, no version bump
    assert len(product_lib.ABI_SYMBOLS) == 103
    out = subprocess.run(["nm", "-D", "--defined-only", str(product_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert exported == sorted(product_lib.ABI_SYMBOLS)


def test_the_wrappers_have_the_switch(product_lib):
    sig = inspect.signature(product_lib.NBodyIntegration.__init__)
    assert sig.parameters["compensated"].default is False
    assert product_lib.NBodyIntegration.compensated is False
    from ephemeris_explorer_amd import ConvergenceError, convergence
    assert list(inspect.signature(convergence).parameters) == ["pos", "vel", "mu", "t0", "bound", "method", "h0"]
    assert inspect.signature(convergence).parameters["h0"].default == 75.0
    assert issubclass(ConvergenceError, Exception)
    hpp = (ROOT / "include" / "ephemeris_amd.hpp").read_text()
    assert "bool compensated = false" in hpp and '"<Double>"' in hpp and "bool compensated() const" in hpp


def test_convergence_example_compiles_and_links(product_lib, tmp_path):
    """examples/convergence.cpp against the product alone, warning-free (the flags of its siblings); without a device its first
    compute call throws Error{EPH_ERR_NO_DEVICE} (exit 77); with one, a 40-day sweep of the three-body system ends with an answer."""
    libdir = ROOT / "ephemeris_explorer_amd"
    exe = tmp_path / "convergence_cpp"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                           str(ROOT / "examples" / "convergence.cpp"), f"-L{libdir}", "-lephemeris_amd",
                           f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    r = subprocess.run([str(exe), str(SYSTEMS / "sun_earth_moon_2433282.5"), "QuinlanTremaine12", "40", "75"], capture_output=True, text=True)
    if product_lib.device_count() < 1:
        assert r.returncode == 77 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 0 and "3 bodies" in r.stdout and "converged at h =" in r.stdout, (r.stdout, r.stderr)


def test_method_name_parser(tmp_path):
    """csrc/method_name.h on its own (tests/method_name_check.cpp): base name + the exact suffix, and every input that must be
    refused -- empty, over-long, unterminated-looking, other suffixes."""
    exe = tmp_path / "method_name_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'ephemeris_explorer_amd' / 'csrc'}",
                           str(ROOT / "tests" / "method_name_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "method_name: ok" in r.stdout, (r.stdout, r.stderr)
