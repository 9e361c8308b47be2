"""The per-cell code of the cell-block right-hand side on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer:
csrc/zzz_mf_elem.h (mf_rhs_mass, mf_rhs_mass3, mf_rhs_facet) and csrc/zzz_cell_geom.h (geometry for |det J|, facet_vertices and
facet_scale_of for the facet's three refetched vertices) -- what a lane of k_mf_rhs runs -- are host-compilable, and
tools/mf_rhs_host.cpp (a stand-alone program with its own main) runs it cell by cell over the cubes below.  The element
vectors it writes, scattered in numpy with the constrained rows zeroed, must be the oracle's vector within 1e-12 max|b|, the
project's bar for assembled values.  The Poisson cases run once more with g == 0: the rows on the Neumann faces must change,
so the facet term is exercised."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zzz
import zzz_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin", "clang++")
ND = {1: 4, 2: 10, 3: 20}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang++ not available")
    exe = str(tmp_path_factory.mktemp("mf_rhs_host") / "mf_rhs_host")
    src = os.path.join(ROOT, "performance-test_amd", "tools", "mf_rhs_host.cpp")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-divide-by-zero", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "performance-test_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(program, tmp_path, P, order, bs, f, g):
    """the program's element vectors scattered, constrained rows zeroed"""
    mask = np.zeros(len(P.cells), np.uint8)
    if bs == 1:
        np.bitwise_or.at(mask, P.facets[:, 0], (1 << P.facets[:, 1]).astype(np.uint8))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        np.array([order, len(P.cells), P.n_owned + P.n_ghost, bs], np.int32).tofile(fh)
        np.ascontiguousarray(P.x[P.cells], np.float64).tofile(fh)
        np.ascontiguousarray(P.cell_dofs, np.int32).tofile(fh)
        mask.tofile(fh)
        np.ascontiguousarray(f, np.float64).tofile(fh)
        if bs == 1:
            np.ascontiguousarray(g, np.float64).tofile(fh)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report goes to stderr and ends the run)
    ye = np.fromfile(fout, np.float64).reshape(len(P.cells), ND[order], bs)
    rows = (P.cell_dofs[:, :, None].astype(np.int64) * bs + np.arange(bs)).reshape(-1)
    b = np.zeros((P.n_owned + P.n_ghost) * bs)
    np.add.at(b, rows, ye.reshape(-1))
    b = b[:P.n_owned * bs]
    b[P.bc_marker().astype(bool)] = 0.0
    return b


CASES = [("poisson", 1, (12, 10, 14)), ("poisson", 2, (6, 5, 7)), ("poisson", 3, (4, 3, 5)),
         ("elasticity", 1, (6, 5, 5)), ("elasticity", 2, (3, 3, 4)), ("elasticity", 3, (2, 2, 3))]


@pytest.mark.parametrize("problem,order,dims", CASES, ids=[f"{p}-P{o}" for p, o, _ in CASES])
def test_host_program_under_sanitizers_gives_the_oracles_vector(program, tmp_path, problem, order, dims):
    zo.set_num_threads(1)
    P = zzz.Part(problem, order, *dims)
    bs = 3 if problem == "elasticity" else 1
    form = zzz.FORM_ELASTICITY if bs == 3 else zzz.FORM_POISSON
    assert P.n_ghost == 0
    if bs == 1:
        ob = zo.assemble_vector(form, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, P.bc_marker())
    else:
        ob = zo.assemble_vector(form, order, P.x, P.cells, P.cell_dofs, P.f, None, None, P.bc_marker())
    b = _run(program, tmp_path, P, order, bs, P.f, P.g if bs == 1 else None)
    err = np.abs(b - ob).max() / np.abs(ob).max()
    print(f"{problem} P{order} {dims}: |b - oracle| / max|b| = {err:.3e}")
    assert err <= 1e-12
    assert np.all(b[P.bc_marker().astype(bool)] == 0.0)
    if bs == 1:
        # g == 0: the rows of the dofs on the exterior facets that were uploaded, and only those, change
        b0 = _run(program, tmp_path, P, order, bs, P.f, np.zeros_like(P.g))
        changed = b0 != b
        on_facet = np.zeros(P.n_owned, bool)
        on_facet[P.cell_dofs[P.facets[:, 0]].reshape(-1)] = True  # (dofs of the cells that hold such a facet: a superset)
        free = ~P.bc_marker().astype(bool)
        assert len(P.facets) > 0 and changed.any() and not changed[~on_facet].any()
        ob0 = zo.assemble_vector(form, order, P.x, P.cells, P.cell_dofs, P.f, np.zeros_like(P.g), P.facets, P.bc_marker())
        assert np.array_equal(changed & free, (ob0 != ob) & free)
        assert np.abs(b0 - ob0).max() <= 1e-12 * np.abs(ob).max()
