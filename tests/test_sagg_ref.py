"""The restatement of ZZZ_PC_SAGG (tests/_sagg_ref.py) pinned on the CPU: its written sums against scipy's products, what the
rule promises (the aggregates of ZZZ_PC_AGG on level 0, symmetric positive definite coarse matrices on the structural pattern, a
symmetric V-cycle), its PCG iteration counts beside plain aggregation's and Jacobi's, and the spread of those counts under
rounding alone (MEASURED_SPREAD).

Bars: a written sum against scipy's product, and the symmetry of a coarse matrix, 1e-13 of the matrix's largest entry (each
entry is a sum of a few hundred to a few thousand terms of mixed sign, scipy adds the same terms in another order); symmetry of
the cycle 1e-12 relative on noise (tests/test_gpu_mg.py's bar)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import _agg_ref as AR
import _sagg_ref as R
from _mg_ref import pcg as pcg_mg
from _pipecg_ref import dot_chunks_reversed

_H, _HA = {}, {}


def hierarchy(name):
    if name not in _H:
        A, bc, _, bs = R.case_system(name)
        _H[name] = R.SaggHierarchy(A, bc, bs, limit=R.LIMIT)
    return _H[name]


def plain(name):
    if name not in _HA:
        A, bc, _, bs = R.case_system(name)
        _HA[name] = AR.AggHierarchy(A, bc, bs, limit=R.LIMIT)
    return _HA[name]


def _ones(M):
    return sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)


def _same_pattern(M, B):
    B = sp.csr_matrix(B)
    B.sort_indices()
    return np.array_equal(M.indptr, B.indptr) and np.array_equal(M.indices, B.indices)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_written_sums_against_scipy(name):
    H = hierarchy(name)
    bs = H.bs
    assert len(H.A) >= 3, [a.shape[0] for a in H.A]
    assert np.array_equal(H.agg[0], plain(name).agg[0]), "level 0 has the aggregates of plain aggregation"
    for l, P in enumerate(H.P):
        A, bc, Ac, T = H.A[l], H.bc[l], H.A[l + 1], H.T[l]
        nagg = Ac.shape[0] // bs
        F = sp.diags((bc == 0).astype(float))
        Pt = AR.prolongator(H.agg[l], bc, bs, nagg)
        omega = 4.0 / (3.0 * H.hi[l])
        Af = (F @ A @ F).tocsr()
        ref = (Pt - omega * (sp.diags(1.0 / A.diagonal()) @ Af @ Pt)).tocsr()
        assert abs(P - ref).max() <= 1e-13 * abs(P).max()
        assert abs(T - F @ A @ P).max() <= 1e-13 * abs(T).max()
        assert abs(Ac - P.T @ A @ P).max() <= 1e-13 * abs(Ac).max()
        assert abs(Ac - Ac.T).max() <= 1e-13 * abs(Ac).max()
        # the patterns are the structural ones: explicit zeros of A count, cancellation removes nothing
        Ab = F @ _ones(A) @ F
        assert _same_pattern(P, Ab @ Pt) and _same_pattern(T, F @ _ones(A) @ _ones(P)) and _same_pattern(Ac, _ones(P).T @ _ones(T))
        assert np.array_equal(np.diff(P.indptr) == 0, bc != 0), "exactly the constrained rows of P are empty"
        scipy.linalg.cholesky(Ac.toarray())  # raises unless positive definite
        # the same sums back to front differ by rounding alone
        D = H.descending()
        assert _same_pattern(P, D.P[l]) and _same_pattern(Ac, D.A[l + 1])
        assert abs(P - D.P[l]).max() <= 1e-13 * abs(P).max() and abs(Ac - D.A[l + 1]).max() <= 1e-13 * abs(Ac).max()
    rows = [int(np.diff(p.indptr).max()) for p in H.P]
    print(f"sagg {name}: dofs {[a.shape[0] for a in H.A]}, nonzeros {[a.nnz for a in H.A]}, longest rows of P {rows}, "
          f"operator complexity {H.complexity():.3f} (plain aggregation {plain(name).complexity():.3f})")


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_cycle_is_symmetric_and_counts_beat_plain_aggregation(name):
    H, HA = hierarchy(name), plain(name)
    A, _, b, _ = R.case_system(name)
    rng = np.random.default_rng(5)
    r, s = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    Mr, Ms = H.vcycle(r), H.vcycle(s)
    sym = abs(Mr @ s - r @ Ms) / (np.linalg.norm(Mr) * np.linalg.norm(s))
    alt = np.abs(H.vcycle_reversed(r) - Mr).max() / np.abs(Mr).max()
    print(f"sagg {name}: symmetry defect {sym:.2e}, difference between the two summation orders {alt:.2e} of max |z|")
    assert sym <= 1e-12 and Mr @ r > 0.0 and Ms @ s > 0.0
    assert alt <= 1e-10
    dj = 1.0 / A.diagonal()
    itj, xj, _ = pcg_mg(A, b, lambda v: dj * v, rtol=1e-8)
    spread = 0
    for norm in (0, 1, 2):
        it, x = R.pcg(A, b, H.vcycle, norm_type=norm, rtol=1e-8)
        it2, _ = R.pcg(A, b, H.vcycle_reversed, norm_type=norm, rtol=1e-8, dot=dot_chunks_reversed)
        ita, _ = R.pcg(A, b, HA.vcycle, norm_type=norm, rtol=1e-8)
        print(f"sagg {name} norm {norm}: restatement {it} iterations ({it2} with every level reversed and the sums in reversed "
              f"chunks), plain aggregation {ita}, jacobi {itj}")
        spread = max(spread, abs(it - it2))
        assert it <= ita < itj
        if name in ("poisson_p1", "elasticity_p1"):
            assert it <= ita - 3
        assert np.linalg.norm(x - xj) <= 1e-6 * np.linalg.norm(xj)
    assert spread <= R.MEASURED_SPREAD


def test_a_larger_cube_needs_hardly_more_iterations():
    import zzz
    import zzz_oracle as zo

    A, _, b, _ = R.case_system("poisson_p1")
    small = R.pcg(A, b, hierarchy("poisson_p1").vcycle, rtol=1e-8)[0]
    P = zzz.Part("poisson", 1, 24, 20, 28)
    zo.set_num_threads(4)
    bc = P.bc_marker()
    rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
    v = zo.assemble_matrix(P.form, P.order, P.x, P.cells, P.cell_dofs, bc, rp, cl)
    b2 = zo.assemble_vector(P.form, P.order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, bc)
    A2 = sp.csr_matrix((v, cl, rp), shape=(rp.size - 1, rp.size - 1))
    H2 = R.SaggHierarchy(A2, bc, 1, limit=1000)
    large = R.pcg(A2, b2, H2.vcycle, rtol=1e-8)[0]
    print(f"sagg poisson P1: 12x10x14 at limit {R.LIMIT} {small} iterations, 24x20x28 ({A2.shape[0]} dofs, levels "
          f"{[a.shape[0] for a in H2.A]}) at limit 1000 {large}")
    assert large <= small + 3


def test_level_rule():
    A, bc, _, bs = R.case_system("poisson_p1")
    assert len(R.SaggHierarchy(A, bc, bs, limit=R.LIMIT, max_levels=2).A) == 2
    assert len(R.SaggHierarchy(A, bc, bs, limit=10**6).A) == 1
    H = R.SaggHierarchy(sp.identity(60, format="csr"), np.ones(60, np.uint8), 1, limit=R.LIMIT)
    assert len(H.A) == 1
