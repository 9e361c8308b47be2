"""The restatement of the geometric multigrid preconditioner (tests/_mg_ref.py) pinned by mathematics, before anything on
the GPU is compared with it: the transfer reproduces linear functions and equals the nested interpolation when nf = 2 nc,
restriction is its adjoint, the V-cycle is a symmetric positive definite operator, and KSPCG around it needs a few
iterations where Jacobi needs hundreds.  One test checks the ABI: the four zzz_mg_* entry points are declared and exported."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import zzz
import zzz_oracle as zo
from _mg_ref import Hierarchy, csr, level_dims, oracle_problem, pcg, prolongation


def vertex_coords(n):
    px, py, pz = (v + 1 for v in n)
    iz, iy, ix = np.meshgrid(np.arange(pz), np.arange(py), np.arange(px), indexing="ij")
    return np.stack([ix.ravel() / n[0], iy.ravel() / n[1], iz.ravel() / n[2]], 1)


@pytest.mark.parametrize("nf,nc", [((7, 6, 5), (4, 3, 3)), ((8, 8, 8), (4, 4, 4))])
def test_prolongation_reproduces_linear_functions(nf, nc):
    assert level_dims(nf, 1, limit=1)[1] == nc
    # the oracle numbers P1 dofs as the restatement numbers vertices
    assert np.abs(oracle_problem("poisson", nf).dof_x - vertex_coords(nf)).max() <= 1e-15
    P = prolongation(nf, nc)
    xf, xc = vertex_coords(nf), vertex_coords(nc)
    for coef in ((1.0, 0.0, 0.0, 0.0), (0.3, 1.0, -2.0, 0.5), (-1.0, 0.25, 0.5, 3.0)):
        lin = lambda x: coef[0] + x @ np.array(coef[1:])
        assert np.abs(P @ lin(xc) - lin(xf)).max() <= 1e-14
    assert np.abs(P.sum(axis=1).A1 - 1.0).max() <= 1e-15 and P.min() >= 0.0


def test_prolongation_is_the_nested_interpolation_when_nf_is_twice_nc():
    nf, nc = (8, 6, 4), (4, 3, 2)
    P = prolongation(nf, nc).toarray()
    pf, pc = [v + 1 for v in nf], [v + 1 for v in nc]
    N = np.zeros_like(P)
    cid = lambda p: (p[2] * pc[1] + p[1]) * pc[0] + p[0]
    for iz in range(pf[2]):
        for iy in range(pf[1]):
            for ix in range(pf[0]):
                i = (ix, iy, iz)
                row = (iz * pf[1] + iy) * pf[0] + ix
                lo = [v // 2 for v in i]
                odd = [v % 2 for v in i]
                hi = [lo[a] + odd[a] for a in range(3)]
                # a fine vertex is a coarse vertex or the midpoint of the coarse Kuhn edge from lo to lo + odd
                N[row, cid(lo)] += 0.5
                N[row, cid(hi)] += 0.5
    assert np.array_equal(P, N)


@pytest.mark.parametrize("kind,n", [("poisson", (6, 5, 4)), ("elasticity", (5, 4, 4))])
def test_restriction_is_the_adjoint_and_the_cycle_is_spd(kind, n):
    H = Hierarchy(kind, n, limit=100)
    assert len(H.dims) >= 2
    rng = np.random.default_rng(3)
    for l, P in enumerate(H.P):
        e, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
        assert abs((P @ e) @ r - e @ (P.T @ r)) <= 1e-13 * np.linalg.norm(P @ e) * np.linalg.norm(r)
        bcf, bcc = H.probs[l].bc.astype(bool), H.probs[l + 1].bc.astype(bool)
        assert np.all((P @ e)[bcf] == 0.0) and np.all((P.T @ r)[bcc] == 0.0)
    nn = H.A[0].shape[0]
    M = np.stack([H.vcycle(np.eye(nn)[:, j]) for j in range(nn)], 1)
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0


@pytest.mark.parametrize("kind,n,cap", [("poisson", (45, 43, 41), 12), ("elasticity", (35, 33, 31), 16)])
def test_iteration_counts(kind, n, cap):
    H = Hierarchy(kind, n)
    p = H.probs[0]
    it, x, hist = pcg(H.A[0], p.b, H.vcycle, rtol=1e-8)
    itj, xj, _, _ = zo.pcg(p.rowptr.astype(np.int64), p.cols, p.vals, p.b, rtol=1e-8)
    _, xt, _, _ = zo.pcg(p.rowptr.astype(np.int64), p.cols, p.vals, p.b, rtol=1e-12)
    print(f"mg_ref {kind} {n}: levels {H.dims}, bounds {H.hi}, mg-pcg {it}, jacobi-pcg {itj}, "
          f"|x-xt|/|xt| {np.linalg.norm(x - xt) / np.linalg.norm(xt):.2e}")
    assert it <= cap
    assert 10 * it < itj
    assert hist.shape[0] == it + 1
    assert np.linalg.norm(x - xt) <= 1e-6 * np.linalg.norm(xt)


def test_norm_types_and_one_level():
    H = Hierarchy("poisson", (12, 10, 14))
    p = H.probs[0]
    its = [pcg(H.A[0], p.b, H.vcycle, norm_type=k)[0] for k in (0, 1, 2)]
    assert max(its) <= 12 and min(its) >= 3
    H1 = Hierarchy("poisson", (4, 4, 4))
    assert len(H1.dims) == 1
    assert pcg(H1.A[0], H1.probs[0].b, H1.vcycle)[0] <= 2
    assert level_dims((216, 206, 222), 1) == [(216, 206, 222), (108, 103, 111), (54, 52, 56), (27, 26, 28), (14, 13, 14), (7, 7, 7)]
    assert len(level_dims((45, 43, 41), 1, max_levels=2)) == 2
    assert level_dims((12, 10, 14), 1, limit=200)[-1] == (3, 3, 4)


def test_abi_declares_and_exports_the_multigrid_entry_points():
    names = ["zzz_mg_setup", "zzz_mg_info", "zzz_mg_apply", "zzz_mg_transfer"]
    for n in names:
        assert n in zzz.ABI_SYMBOLS
    header = open(os.path.join(zzz.ROOT, "include", "zzz_abi.h")).read()
    assert "#define ZZZ_ABI_VERSION 7" in header and "ZZZ_PC_MG = 3" in header and zzz.PC_MG == 3
    out = subprocess.run(["nm", "-D", "--defined-only", zzz.hip_lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n in exported
    # the options struct grew behind its existing fields
    f = [name for name, _ in zzz.SolverOpts._fields_]
    assert f[-2:] == ["pc_mg_levels", "pc_mg_coarse_eq_limit"] and f.index("pc_ratio") == len(f) - 3
