"""The restatement of ZZZ_PC_SAGG_RBM (tests/_sagg_rbm_ref.py) pinned on the CPU, on the three elasticity cases of
tests/_agg_ref.py and on the island case (elasticity P1 6 x 6 x 6 with every node of x-index >= 4 constrained except one
isolated node and one pair: aggregates whose rigid-body modes are dependent): what the rule promises -- an orthonormal
tentative prolongator that reproduces the near-nullspace on every level, symmetric positive definite coarse matrices, a
symmetric V-cycle, a clear gap between kept and dropped columns -- its PCG iteration counts beside ZZZ_PC_SAGG's, and the spread
of those counts under rounding alone (MEASURED_SPREAD).

Bars: orthonormality and the symmetry of a coarse matrix 1e-13 (of the matrix's largest entry); P_t B_c against B 1e-12 of B's
largest entry; symmetry of the cycle 1e-12 relative on noise (tests/test_gpu_mg.py's bar); no orthogonalisation ratio between
2^-40 and 2^-20, so that rounding cannot flip a drop (the threshold is 2^-30) between the restatement and the library."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import zzz_oracle as zo
import _sagg_ref as SR
import _sagg_rbm_ref as R
from _mg_ref import pcg as pcg_mg
from _pipecg_ref import dot_chunks_reversed

NAMES = R.ELASTICITY + ["island"]
_S, _H, _HS = {}, {}, {}


def system(name):
    """(A, bc, b, B): the case's system from the oracle and six rigid-body modes at its dof coordinates"""
    if name not in _S:
        if name == "island":
            P = R.case_part("elasticity_p1")
            bc, _ = R.island_bc(P)
            zo.set_num_threads(4)
            rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
            v = zo.assemble_matrix(P.form, P.order, P.x, P.cells, P.cell_dofs, bc, rp, cl)
            b = zo.assemble_vector(P.form, P.order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, bc)
            A = sp.csr_matrix((v, cl, rp), shape=(rp.size - 1, rp.size - 1))
        else:
            P = R.case_part(name)
            A, bc, b, _ = R.case_system(name)
        _S[name] = (A, bc, b, R.rigid_body_modes(P.dof_x, P.n_owned))
    return _S[name]


def hierarchy(name):
    if name not in _H:
        A, bc, _, B = system(name)
        _H[name] = R.RbmHierarchy(A, bc, B, limit=R.LIMIT)
    return _H[name]


def sagg(name):
    if name not in _HS:
        A, bc, _, _ = system(name)
        _HS[name] = SR.SaggHierarchy(A, bc, 3, limit=R.LIMIT)
    return _HS[name]


@pytest.mark.parametrize("name", NAMES)
def test_what_the_rule_promises(name):
    H = hierarchy(name)
    D = H.descending()
    assert len(H.A) >= 3, [a.shape[0] for a in H.A]
    for l, P in enumerate(H.P):
        A, bc, Ac, Pt, keep, B, Bc = H.A[l], H.bc[l], H.A[l + 1], H.Pt[l], H.keep[l], H.B[l], H.B[l + 1]
        G = (Pt.T @ Pt).toarray()
        assert np.abs(G - np.diag(keep.astype(float))).max() <= 1e-13, "P_t^T P_t: the identity on kept columns, 0 on dropped ones"
        assert np.all(Bc.T[~keep] == 0.0), "row q of R is 0 for a dropped column"
        assert np.abs(Pt @ Bc.T - B.T).max() <= 1e-12 * np.abs(B).max(), "P_t B_c reproduces B with constrained rows zeroed"
        assert np.all(B[:, bc != 0] == 0.0)
        assert abs(Ac - Ac.T).max() <= 1e-13 * abs(Ac).max()
        scipy.linalg.cholesky(Ac.toarray())  # raises unless positive definite
        assert np.array_equal(np.diff(P.indptr) == 0, bc != 0), "exactly the constrained rows of P are empty"
        assert np.all(np.diff(P.tocsc().indptr)[~keep] == 0), "a dropped coarse dof has no entry in P"
        d = np.flatnonzero(~keep)
        assert np.all(np.diff(Ac.indptr)[d] == 1) and np.all(Ac.diagonal()[d] == 1.0), "its row of A_c is the unit diagonal"
        # the written sums against scipy's products
        omega = 4.0 / (3.0 * H.hi[l])
        F = sp.diags((bc == 0).astype(float))
        ref = (Pt - omega * (sp.diags(1.0 / A.diagonal()) @ (F @ A @ F) @ Pt)).tocsr()
        assert abs(P - ref).max() <= 1e-13 * abs(P).max()
        U = sp.diags((~keep).astype(float))
        assert abs(Ac - (P.T @ A @ P + U)).max() <= 1e-13 * abs(Ac).max()
        # no ratio near the threshold: a drop is the same decision under any rounding
        r = H.ratios[l]
        assert not np.any((r > 2.0 ** -40) & (r < 2.0 ** -20)), r[(r > 2.0 ** -40) & (r < 2.0 ** -20)]
        assert np.array_equal(keep, D.keep[l])
        assert abs(P - D.P[l]).max() <= 1e-13 * abs(P).max() and abs(Ac - D.A[l + 1]).max() <= 1e-13 * abs(Ac).max()
        kept = r[keep]
        print(f"sagg_rbm {name} level {l}: {A.shape[0]} -> {Ac.shape[0]} dofs, {int((~keep).sum())} dropped, smallest kept ratio "
              f"{kept.min():.3g}, largest dropped {r[~keep].max() if (~keep).any() else 0.0:.3g}, rows of P up to "
              f"{int(np.diff(P.indptr).max())}")
    print(f"sagg_rbm {name}: dofs {[a.shape[0] for a in H.A]}, dropped {H.dropped()}, operator complexity {H.complexity():.3f}")
    if name == "island":
        assert [a.shape[0] for a in H.A] == [1029, 78, 18] and H.dropped() == [0, 4, 4]
        per = (~H.keep[0]).reshape(-1, 6).sum(axis=1)
        assert sorted(per[per > 0]) == [1, 3], "a collinear pair drops one column, a single free node three"


@pytest.mark.parametrize("name", NAMES)
def test_cycle_is_symmetric_and_counts_beat_sagg(name):
    H, HS = hierarchy(name), sagg(name)
    A, _, b, _ = system(name)
    rng = np.random.default_rng(5)
    r, s = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    Mr, Ms = H.vcycle(r), H.vcycle(s)
    sym = abs(Mr @ s - r @ Ms) / (np.linalg.norm(Mr) * np.linalg.norm(s))
    alt = np.abs(H.vcycle_reversed(r) - Mr).max() / np.abs(Mr).max()
    print(f"sagg_rbm {name}: symmetry defect {sym:.2e}, difference between the two summation orders {alt:.2e} of max |z|")
    assert sym <= 1e-12 and Mr @ r > 0.0 and Ms @ s > 0.0
    assert alt <= 1e-10
    dj = 1.0 / A.diagonal()
    itj, xj, _ = pcg_mg(A, b, lambda v: dj * v, rtol=1e-8)
    spread = 0
    for norm in (0, 1, 2):
        it, x = R.pcg(A, b, H.vcycle, norm_type=norm, rtol=1e-8)
        it2, _ = R.pcg(A, b, H.vcycle_reversed, norm_type=norm, rtol=1e-8, dot=dot_chunks_reversed)
        its, _ = R.pcg(A, b, HS.vcycle, norm_type=norm, rtol=1e-8)
        print(f"sagg_rbm {name} norm {norm}: restatement {it} iterations ({it2} with every level reversed and the sums in "
              f"reversed chunks), sagg {its}, jacobi {itj}")
        spread = max(spread, abs(it - it2))
        assert it < its < itj, "strictly below ZZZ_PC_SAGG's count"
        assert np.linalg.norm(x - xj) <= 1e-6 * np.linalg.norm(xj)
    assert spread <= R.MEASURED_SPREAD


def test_the_one_sum_and_the_level_rule():
    v = np.random.default_rng(1).standard_normal(333)
    assert abs(R.wave_sum(v) - v.sum()) <= 1e-13 and abs(R.wave_sum(v, True) - v.sum()) <= 1e-13
    assert R.wave_sum(np.arange(200.0)) == 19900.0 and R.wave_sum(np.zeros(0)) == 0.0
    A, bc, _, B = system("elasticity_p1")
    assert len(R.RbmHierarchy(A, bc, B, limit=R.LIMIT, max_levels=2).A) == 2
    assert len(R.RbmHierarchy(A, bc, B, limit=10**6).A) == 1
