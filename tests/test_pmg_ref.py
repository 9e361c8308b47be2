"""The restatement of the p-multigrid preconditioner (tests/_pmg_ref.py) pinned by mathematics, before anything on the GPU is
compared with it: the transfer built from "P1 basis at the Pk dof points" reproduces linear functions at the Pk dof
coordinates, its rows are convex combinations, restriction is its adjoint, the cycle is a symmetric positive definite operator,
and KSPCG around it needs about a dozen iterations where Jacobi needs hundreds.

Iteration caps: the counts measured on this restatement with the oracle's bounds, degree 2, ratio 10, rtol 1e-8 (8, 13, 12 and
24 for the four cases below) plus half, so a slip that costs a third more iterations fails while a last-bit difference that
moves the count by one does not.  One test checks the ABI: the enumerator is there and the version did not move."""
import os

import numpy as np
import pytest
import zzz
import zzz_oracle as zo
from _mg_ref import pcg
from _pmg_ref import PHierarchy, part, pmg_level_dims, prolongation


@pytest.mark.parametrize("kind,order,n", [("poisson", 2, (4, 3, 5)), ("poisson", 3, (3, 2, 4)), ("elasticity", 3, (3, 2, 3))])
def test_prolongation_reproduces_linear_functions_and_is_convex(kind, order, n):
    P, spread = prolongation(kind, order, n)
    F, C = part(kind, order, n), part(kind, 1, n)
    assert spread <= 1e-15  # two cells that share a dof agree on its row
    xf, xc = F.dof_x[:F.n_owned], C.dof_x[:C.n_owned]
    assert np.array_equal(xc, C.x)  # the P1 dofs are the feed's vertices, in their order
    for coef in ((1.0, 0.0, 0.0, 0.0), (0.3, 1.0, -2.0, 0.5), (-1.0, 0.25, 0.5, 3.0)):
        lin = lambda x: coef[0] + x @ np.array(coef[1:])
        assert np.abs(P @ lin(xc) - lin(xf)).max() <= 1e-14
    assert np.abs(P.sum(axis=1).A1 - 1.0).max() <= 1e-15 and P.min() >= 0.0
    # 1 term at a vertex, 2 on an edge, 3 at a face centroid
    per_row = np.diff(P.indptr)
    assert set(per_row) == ({1, 2} if order == 2 else {1, 2, 3})
    assert (per_row == 1).sum() == C.n_owned


@pytest.mark.parametrize("kind,order,n", [("poisson", 3, (3, 2, 4)), ("elasticity", 2, (3, 2, 3))])
def test_restriction_is_the_adjoint_and_the_cycle_is_spd(kind, order, n):
    H = PHierarchy(kind, order, n, limit=50)
    assert len(H.dims) >= 3 and H.dims == pmg_level_dims(n, H.bs, limit=50)
    rng = np.random.default_rng(5)
    P = H.P
    e, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
    assert abs((P @ e) @ r - e @ (P.T @ r)) <= 1e-13 * np.linalg.norm(P @ e) * np.linalg.norm(r)
    bcf, bcc = H.bc.astype(bool), H.H1.probs[0].bc.astype(bool)
    assert bcf.any() and bcc.any()
    assert np.all((P @ e)[bcf] == 0.0) and np.all((P.T @ r)[bcc] == 0.0)
    assert abs(P[bcf]).sum() == 0.0 and abs(P[:, bcc]).sum() == 0.0
    nn = H.A.shape[0]
    M = np.stack([H.vcycle(np.eye(nn)[:, j]) for j in range(nn)], 1)
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0


@pytest.mark.parametrize("kind,order,n,cap", [("poisson", 2, (12, 10, 14), 12), ("poisson", 3, (8, 7, 9), 19),
                                              ("elasticity", 2, (10, 9, 8), 18), ("elasticity", 3, (6, 5, 7), 36)])
def test_iteration_counts(kind, order, n, cap):
    H = PHierarchy(kind, order, n)
    it, x, hist = pcg(H.A, H.b, H.vcycle, rtol=1e-8)
    itj, _, _, _ = zo.pcg(H.rowptr, H.cols, H.vals, H.b, rtol=1e-8)
    _, xt, _, _ = zo.pcg(H.rowptr, H.cols, H.vals, H.b, rtol=1e-12)
    err = np.linalg.norm(x - xt) / np.linalg.norm(xt)
    print(f"pmg_ref {kind} P{order} {n}: levels {H.dims}, bounds {H.hi}, pmg-pcg {it}, jacobi-pcg {itj}, |x-xt|/|xt| {err:.2e}")
    assert it <= cap
    assert 10 * it < itj
    assert hist.shape[0] == it + 1
    assert err <= 1e-6


def test_level_rule():
    assert pmg_level_dims((12, 10, 14), 1) == [(12, 10, 14), (12, 10, 14), (6, 5, 7)]
    assert pmg_level_dims((4, 3, 5), 1) == [(4, 3, 5), (4, 3, 5)]
    assert pmg_level_dims((12, 10, 14), 1, max_levels=2) == [(12, 10, 14), (12, 10, 14)]
    assert pmg_level_dims((6, 5, 7), 3, limit=200) == [(6, 5, 7), (6, 5, 7), (3, 3, 4), (2, 2, 2)]


def test_abi_has_the_enumerator_and_keeps_its_version():
    header = open(os.path.join(zzz.ROOT, "include", "zzz_abi.h")).read()
    assert "ZZZ_PC_PMG = 4" in header and zzz.PC_PMG == 4
    assert "ZZZ_PC_MG = 3" in header and zzz.PC_MG == 3
    assert "#define ZZZ_ABI_VERSION 7" in header
