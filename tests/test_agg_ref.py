"""The restatement of ZZZ_PC_AGG (tests/_agg_ref.py) pinned on the CPU: what the rule promises (a partition of the
unconstrained nodes, roots more than distance 2 apart, symmetric positive definite coarse matrices, a symmetric V-cycle), its
PCG iteration counts beside Jacobi's, and the spread of those counts under rounding alone (MEASURED_SPREAD).

Bars: symmetry of a coarse matrix 1e-13 of its largest entry (each entry is a sum of a few hundred terms, its transpose the
same terms in another order); symmetry of the cycle 1e-12 relative on noise (tests/test_gpu_mg.py's bar)."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import _agg_ref as R
from _mg_ref import pcg as pcg_mg
from _pipecg_ref import dot_chunks_reversed

_H = {}


def hierarchy(name):
    if name not in _H:
        A, bc, _, bs = R.case_system(name)
        _H[name] = R.AggHierarchy(A, bc, bs, limit=R.LIMIT)
    return _H[name]


def test_priority_is_the_written_formula():
    # the formula once more, in Python integers reduced modulo 2^64
    x = (0 + 0x9E3779B97F4A7C15) & (2**64 - 1)
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) % 2**64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) % 2**64
    x ^= x >> 31
    assert R.priority(0) == (x >> 33) << 32
    keys = [R.priority(i) for i in range(4096)]
    assert len(set(keys)) == 4096 and all(0 <= k < 2**63 and (k & 0xffffffff) == i for i, k in enumerate(keys))


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_aggregates_roots_and_coarse_matrices(name):
    H = hierarchy(name)
    bs = H.bs
    assert len(H.A) >= 3, [a.shape[0] for a in H.A]
    for l, agg in enumerate(H.agg):
        A, bc = H.A[l], H.bc[l]
        n = A.shape[0] // bs
        free, ei, ej = R.node_edges(A, bc, bs)
        nagg = H.A[l + 1].shape[0] // bs
        # every unconstrained node is in exactly one aggregate, nobody else is in any, no aggregate is empty
        assert np.all(agg[free] >= 0) and np.all(agg[~free] == -1) and agg.max() == nagg - 1
        assert np.array_equal(np.unique(agg[free]), np.arange(nagg))
        # aggregates are connected to their root within distance 2, numbered by ascending root
        roots = H.roots[l]
        assert np.all(np.diff(roots) > 0) and np.array_equal(agg[roots], np.arange(roots.size))
        G = sp.csr_matrix((np.ones(ei.size), (ei, ej)), shape=(n, n)) + sp.identity(n)
        G2 = (G @ G).tocsr()
        sub = G2[roots][:, roots].tocoo()
        assert np.all(sub.row == sub.col), "two roots within distance 2"
        # ... and the set is maximal: every graph node has a root within distance 2
        reach = np.asarray(G2[:, roots].sum(axis=1)).ravel()
        assert np.all(reach[free] > 0)
        # P has one unit entry in each unconstrained row
        P = H.P[l]
        assert np.array_equal(np.asarray(P.sum(axis=1)).ravel(), (bc == 0).astype(float))
    for l in range(1, len(H.A)):
        Ac = H.A[l]
        ref = (H.P[l - 1].T @ H.A[l - 1] @ H.P[l - 1]).tocsr()
        assert abs(Ac - ref).max() <= 1e-13 * abs(Ac).max()
        assert abs(Ac - Ac.T).max() <= 1e-13 * abs(Ac).max()
        scipy.linalg.cholesky(Ac.toarray())  # raises unless positive definite
    print(f"agg {name}: dofs {[a.shape[0] for a in H.A]}, nonzeros {[a.nnz for a in H.A]}, rounds {H.rounds}, "
          f"operator complexity {H.complexity():.3f}")


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_cycle_is_symmetric_and_counts_beat_jacobi(name):
    H = hierarchy(name)
    A, _, b, _ = R.case_system(name)
    rng = np.random.default_rng(5)
    r, s = rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[0])
    Mr, Ms = H.vcycle(r), H.vcycle(s)
    sym = abs(Mr @ s - r @ Ms) / (np.linalg.norm(Mr) * np.linalg.norm(s))
    alt = np.abs(H.vcycle_reversed(r) - Mr).max() / np.abs(Mr).max()
    print(f"agg {name}: symmetry defect {sym:.2e}, difference between the two summation orders {alt:.2e} of max |z|")
    assert sym <= 1e-12 and Mr @ r > 0.0 and Ms @ s > 0.0
    assert alt <= 1e-10
    dj = 1.0 / A.diagonal()
    itj, xj, _ = pcg_mg(A, b, lambda v: dj * v, rtol=1e-8)
    spread = 0
    for norm in (0, 1, 2):
        it, x = R.pcg(A, b, H.vcycle, norm_type=norm, rtol=1e-8)
        it2, _ = R.pcg(A, b, H.vcycle, norm_type=norm, rtol=1e-8, dot=dot_chunks_reversed)
        print(f"agg {name} norm {norm}: restatement {it} iterations ({it2} with the sums in reversed chunks), jacobi {itj}")
        spread = max(spread, abs(it - it2))
        assert it < itj
        assert np.linalg.norm(x - xj) <= 1e-6 * np.linalg.norm(xj)
    assert spread <= R.MEASURED_SPREAD


def test_level_rule():
    A, bc, _, bs = R.case_system("poisson_p1")
    assert len(R.AggHierarchy(A, bc, bs, limit=R.LIMIT, max_levels=2).A) == 2
    assert len(R.AggHierarchy(A, bc, bs, limit=10**6).A) == 1
    # every dof constrained: no graph, one level
    H = R.AggHierarchy(sp.identity(60, format="csr"), np.ones(60, np.uint8), 1, limit=R.LIMIT)
    assert len(H.A) == 1
    # a diagonal-only row among coupled ones is an aggregate of its own
    T = sp.diags([-np.ones(99), 2.0 * np.ones(100), -np.ones(99)], [-1, 0, 1]).tolil()
    T[40, 39] = T[40, 41] = T[39, 40] = T[41, 40] = 0.0
    agg, roots, nagg, _ = R.aggregate(T.tocsr(), np.zeros(100, np.uint8), 1)
    assert 40 in roots and np.sum(agg == agg[40]) == 1
