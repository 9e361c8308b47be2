"""csrc/zzz_sagg_rows.h on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: what the row-by-row products of
ZZZ_MG_PRODUCTS_ROWS (csrc/zzz_sagg_rows.hip) share between kernels and host code is host-compilable, and
tools/sagg_rows_host.cpp (a stand-alone program with its own main) runs it: the chunk partition on empty rows, a total of zero,
a row over the budget, budget 1 and 4 096 rows of 2^20 candidates each (a 2^32 total: the sums must be 64-bit); the search of a
column in sorted rows of 0, 1, 63, 64 and 65 entries; and one small product C = L B formed row by row -- in one chunk, in
several, and with every row a chunk of its own -- against the sorted term list's order, bit for bit."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin", "clang++")


def test_host_program_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang++ not available")
    exe = str(tmp_path / "sagg_rows_host")
    src = os.path.join(ROOT, "performance-test_amd", "tools", "sagg_rows_host.cpp")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "performance-test_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report goes to stderr and ends the run)
    assert r.stdout.count("product: ") == 3 and r.stdout.strip().endswith("ok")
