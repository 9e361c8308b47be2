"""The float action's per-cell code on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: csrc/zzz_mf_elem.h --
the rounding of the geometry factors and reference tables, the block-relative P1 coordinates and the element arithmetic the
kernel's lanes run -- is host-compilable, and tools/mf_f32_host.cpp (a stand-alone program with its own main) runs it over
a P1, a P2 and a P3 cube.  The element vectors it writes, scattered in double, must give the action the numpy restatement
(tests/_f32_ref.py) gives: the same bound as on the GPU, 4 x the restatement's own error against the double action."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _f32_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin", "clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang++ not available")
    exe = str(tmp_path_factory.mktemp("mf_f32_host") / "mf_f32_host")
    src = os.path.join(ROOT, "performance-test_amd", "tools", "mf_f32_host.cpp")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "performance-test_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("order,dims", [(1, (12, 10, 14)), (2, (6, 5, 7)), (3, (4, 3, 5))])
def test_host_program_under_sanitizers_matches_the_restatement(program, tmp_path, order, dims):
    P, Ae, _ = fr.cube(order, dims)
    u = fr.noise(P.n)
    block = 256
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([order, len(P.cells), P.n, block], np.int32).tofile(f)
        np.ascontiguousarray(P.x[P.cells], np.float64).tofile(f)
        np.ascontiguousarray(P.cell_dofs, np.int32).tofile(f)
        u.tofile(f)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report goes to stderr and ends the run)
    ye = np.fromfile(fout, np.float32).reshape(P.cell_dofs.shape)
    y = fr.scatter(P.cell_dofs, ye, P.bc, P.n)
    y64 = fr.action(Ae, P.cell_dofs, P.bc, u, np.float64)
    if order == 1:
        ry = fr.action32_p1_geometry(P.x, P.cells, P.cell_dofs, P.bc, u, chunk=block)
    else:
        ry = fr.action(Ae, P.cell_dofs, P.bc, u, np.float32)
    err = np.abs(y - y64).max() / np.abs(y64).max()
    ref = np.abs(ry - y64).max() / np.abs(y64).max()
    print(f"P{order} {dims}: host program {err:.3e}, restatement {ref:.3e}")
    assert 0 < err <= 4 * ref
