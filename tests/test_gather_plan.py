"""csrc/gather_plan.h, the host side of eph_craft_batch_gather as a pure host value: tests/gather_plan_check.cpp (3000 seeded random
cases of 1 to 5 sources of 0 to 300 craft, with and without burns, dealt and undealt sources, duplicates, empty selections and
concatenations; the merged timeline CSR slice by slice, the per-source lists, the depths and every refusal against a naive model) is
compiled with AddressSanitizer and UBSan and run. No GPU, no HIP: the header compiles with plain g++."""
import re
import subprocess

from conftest import ROOT


def test_gather_plan_model_check(tmp_path):
    exe = tmp_path / "gather_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(ROOT / "tests" / "gather_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"cases (\d+) refusals (\d+) dealt_sources (\d+) duplicates (\d+) empty (\d+) with_burns (\d+)", r.stdout)
    assert m, r.stdout
    cases, refusals, dealt, duplicates, empty, with_burns = map(int, m.groups())
    assert cases >= 3000 and refusals >= 10_000 and dealt >= 500 and duplicates >= 1000 and empty >= 100 and with_burns >= 500, r.stdout
