"""csrc/table_layout.h, the live table's bookkeeping as a pure host value: tests/table_layout_check.cpp (a deque of polynomial ids per
body, one vector of rows for the device, 125 000 seeded random appends / prepends / trims / merges over 1 to 5 bodies, every plan's
uploads executed and the table compared with the model after every operation) is compiled with AddressSanitizer and UBSan and run.
No GPU, no HIP: the header compiles with plain g++."""
import re
import subprocess

from conftest import ROOT


def test_table_layout_model_check(tmp_path):
    exe = tmp_path / "table_layout_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(ROOT / "tests" / "table_layout_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"operations (\d+) fits (\d+) relayouts (\d+)", r.stdout)
    assert m, r.stdout
    operations, fits, relayouts = map(int, m.groups())
    assert operations >= 100_000 and fits >= 100 and relayouts >= 100, r.stdout
