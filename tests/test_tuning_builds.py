"""The tuning builds of the step kernels that every round's evidence uses (csrc/step_wg.hip: EPH_WG_SIDE, EPH_WG_ABLATE;
csrc/step_small.hip: EPH_SMALL_ACCOUNT; all behind -DEPH_EXPERIMENTS=1) still compile, and their switches do nothing to the
product. Device-only compiles of order 0; no GPU."""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from ephemeris_explorer_amd import build as b

TUNING = (["-DEPH_EXPERIMENTS=1", "-DEPH_WG_SIDE=1"], ["-DEPH_EXPERIMENTS=1", "-DEPH_WG_SIDE=3"], ["-DEPH_EXPERIMENTS=1", "-DEPH_WG_ABLATE=3"])
PRODUCT = ([], ["-DEPH_WG_SIDE=1"])          # without EPH_EXPERIMENTS the switch must be inert


SMALL_TUNING = ["-DEPH_EXPERIMENTS=1", "-DEPH_SMALL_ACCOUNT=1"]      # step_small.hip: the per-phase tick accounting of k_lm_small
SMALL_PRODUCT = ([], ["-DEPH_SMALL_ACCOUNT=1"])


def compile_all(tmp, unit, variants):
    """{flags: (exit status, compiler output, assembly text)} of one unit's compiles, run side by side"""
    def one(job):
        i, extra = job
        out = tmp / f"{unit}_{i}.s"
        # (-fuse-cuid=none: the unit's id symbol is a hash of the command line, the one thing a stray -D may change)
        r = subprocess.run([b.hipcc(), *b.FLAGS, "-DEPH_PAIR_VARIANT=0", *extra, "-fuse-cuid=none", "--offload-device-only", "-S", "-x", "hip",
                            str(b.CSRC / f"{unit}.hip"), "-o", str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return tuple(extra), (r.returncode, r.stdout, out.read_text() if out.exists() else "")
    with ThreadPoolExecutor(5) as ex:
        return dict(ex.map(one, enumerate(variants)))


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_all(tmp_path_factory.mktemp("tuning"), "step_wg", [*TUNING, *PRODUCT])


@pytest.fixture(scope="module")
def compiled_small(tmp_path_factory):
    return compile_all(tmp_path_factory.mktemp("tuning_small"), "step_small", [SMALL_TUNING, *SMALL_PRODUCT])


@pytest.mark.parametrize("flags", TUNING, ids=lambda f: f[-1].lstrip("-D"))
def test_tuning_build_compiles(compiled, flags):
    status, log, text = compiled[tuple(flags)]
    assert status == 0, log[-3000:]
    assert ".amdhsa_kernel" in text


def test_switch_is_inert_without_eph_experiments(compiled):
    (s0, log0, plain), (s1, log1, stray) = (compiled[tuple(f)] for f in PRODUCT)
    assert s0 == 0, log0[-3000:]
    assert s1 == 0, log1[-3000:]
    assert ".amdhsa_kernel" in plain
    assert plain == stray, "-DEPH_WG_SIDE=1 alone changed the product's device code"


def test_small_kernel_accounting_build_compiles(compiled_small):
    status, log, text = compiled_small[tuple(SMALL_TUNING)]
    assert status == 0, log[-3000:]
    assert ".amdhsa_kernel" in text


def test_small_kernel_switch_is_inert_without_eph_experiments(compiled_small):
    (s0, log0, plain), (s1, log1, stray) = (compiled_small[tuple(f)] for f in SMALL_PRODUCT)
    assert s0 == 0, log0[-3000:]
    assert s1 == 0, log1[-3000:]
    assert ".amdhsa_kernel" in plain
    assert plain == stray, "-DEPH_SMALL_ACCOUNT=1 alone changed the product's device code"
