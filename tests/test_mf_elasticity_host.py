"""The per-cell code of the matrix-free elasticity action on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer.

csrc/zzz_mf_elem.h holds what the lanes of the block-size-3 kernel run (P1 from the vertex coordinates; P2 / P3 the factorised
form in three phases; the element matrix's diagonal), host-compilable; tools/mf_elast_host.cpp (a stand-alone program with its
own main) runs it over the cubes 3 x 2 x 2 (P1), 2 x 2 x 2 (P2) and 2 x 1 x 2 (P3) and prints the element results.  Summed over
the cells they must give what the oracle's assembled, unconstrained matrix gives: A u for a seeded u through zo.spmv, and A's
diagonal -- both to 1e-12 of the largest reference value, the bar the Poisson action is held to in tests/test_gpu_cg.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zzz_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin", "clang++")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang++ not available")
    exe = str(tmp_path_factory.mktemp("mf_elast_host") / "mf_elast_host")
    src = os.path.join(ROOT, "performance-test_amd", "tools", "mf_elast_host.cpp")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "performance-test_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(program, tmp_path, O, u, diag):
    nd = O.cell_dofs.shape[1]
    fin = str(tmp_path / f"in{diag}.txt")
    with open(fin, "w") as f:
        f.write(f"{O.order} {len(O.cells)} {O.nblock} {diag}\n")
        for arr in (O.x[O.cells].reshape(-1), O.cell_dofs.reshape(-1), u):
            f.write(" ".join(repr(v) for v in arr.tolist()) + "\n")
    r = subprocess.run([program, fin], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report goes to stderr and ends the run)
    ye = np.array([[float(t) for t in line.split()] for line in r.stdout.splitlines()]).reshape(len(O.cells), nd, 3)
    y = np.zeros((O.nblock, 3))
    np.add.at(y, O.cell_dofs, ye)
    return y.reshape(-1)


@pytest.mark.parametrize("order,dims", [(1, (3, 2, 2)), (2, (2, 2, 2)), (3, (2, 1, 2))])
def test_element_results_sum_to_the_assembled_operator(program, tmp_path, order, dims):
    zo.set_num_threads(1)
    O = zo.Problem("elasticity", order, *dims)
    n = O.nblock * 3
    rp, cl = zo.pattern(O.nblock, O.cell_dofs, 3)
    A = zo.assemble_matrix(1, order, O.x, O.cells, O.cell_dofs, np.zeros(n, np.uint8), rp, cl)
    u = np.random.default_rng(5).standard_normal(n)
    oy = zo.spmv(rp, cl, A, u)
    rows = np.repeat(np.arange(n), np.diff(rp))
    od = np.zeros(n)
    od[rows[cl == rows]] = A[cl == rows]
    y = _run(program, tmp_path, O, u, 0)
    d = _run(program, tmp_path, O, u, 1)
    ey, ed = np.abs(y - oy).max() / np.abs(oy).max(), np.abs(d - od).max() / np.abs(od).max()
    print(f"P{order} {dims}: {len(O.cells)} cells, action {ey:.2e}, diagonal {ed:.2e} of the largest reference value")
    assert np.abs(oy).max() > 0 and np.all(od > 0)
    assert ey <= 1e-12
    assert ed <= 1e-12
