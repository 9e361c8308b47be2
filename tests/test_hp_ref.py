"""The 50-digit restatement (tests/_hp_ref.py) against the oracle's element kernels and the golden element tensors, and the
oracle's distance from it on the hostile meshes (tests/_hostile.py): no GPU needed.

The figures of the last test are max |oracle - reference| / scale in units of 2^-53 for the unconstrained Poisson matrix,
with the scale of _hp_ref.py.  Measured when the reference was written (P1 6x5x5, P2 4x4x5, P3 3x3x4 cubes):

    identity, offset, aniso, graded, rotated, needle, noise13   P1   1.0 - 1.8
    aniso                                                       P2   2.2
    graded                                                      P3   5.9
    shear50_a                                                   P1 / P2 / P3   23.6 / 26.3 / 24.9

The oracle sits within a few units of the truth and loses digits only where cond(J) grows.  Each figure must stay within
twice the measured one (for the P1 group: twice the group's worst, 1.8): a change of the oracle that loses digits fails
here, on the CPU, before any kernel is judged against it.
"""
import os

import numpy as np
import pytest

import _hostile
import _hp_ref as hp
import zzz_oracle as zo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _one_thread():
    zo.set_num_threads(1)


def _tets(order):
    rng = np.random.default_rng(100 + order)
    return (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.0]]), rng.random((4, 3)), rng.random((4, 3))[[1, 0, 2, 3]])


@pytest.mark.parametrize("order", [1, 2, 3])
def test_element_tensors_against_the_oracle(order):
    """Poisson matrix, mass and facet tensors of one cell: the oracle integrates by Gauss quadrature in doubles, so it is
    held to 64 units of the entry's scale (nd <= 20 terms per quadrature sum, tens of points)"""
    t = hp.tables(order)
    nd = t["nd"]
    for xc in _tets(order):
        A, sc = hp.element_matrix(order, xc)
        A = np.array([[float(v) for v in row] for row in A])
        Ao = zo.tabulate("poisson_a", order, xc)
        assert hp.metric(Ao, A, sc) <= 64 * hp.U
        adet = hp.geometry(xc)[0]
        M = np.array([[float(adet * v) for v in row] for row in t["M"]])
        Mo = np.array([zo.tabulate("poisson_L", order, xc, w=np.r_[np.eye(nd)[j], np.zeros(nd)]) for j in range(nd)])
        assert np.abs(M - Mo).max() <= 64 * hp.U * np.abs(M).max()
        for lf in range(4):
            s = hp.facet_scale(xc, lf)
            F = np.array([[float(s * v) for v in row] for row in t["F"][lf]])
            Fo = np.array([zo.tabulate("poisson_L_facet", order, xc, w=np.r_[np.zeros(nd), np.eye(nd)[j]], facet=lf)
                           for j in range(nd)])
            assert np.abs(F - Fo).max() <= 64 * hp.U * np.abs(F).max()
            # a dof that is not on the facet takes nothing from it, exactly
            off = [i for i in range(4) if i not in hp.FACE_V[lf]]
            assert np.all(F[off] == 0.0) and np.all(F[:, off] == 0.0)
            # ... in the oracle too (it used to leave ~1e-20 |n| g there, which the scale of a small entry of b does not cover)
            assert np.all(Fo[off] == 0.0) and np.all(Fo[:, off] == 0.0)


def test_element_tensors_against_the_golden_vectors():
    """the golden tensors were integrated by another quadrature in doubles and stored: 1e-13 of the largest entry, their
    own bar in test_element_tables.py"""
    e = np.load(os.path.join(ROOT, "tests", "golden", "element_tensors.npz"))
    for order in (1, 2, 3):
        t = hp.tables(order)
        for nm in ("ref", "tet"):
            A, _ = hp.element_matrix(order, e[nm])
            A = np.array([[float(v) for v in row] for row in A])
            G = e[f"poisson_a_p{order}_{nm}"]
            assert np.abs(A - G).max() <= 1e-13 * np.abs(G).max()
            adet = hp.geometry(e[nm])[0]
            M = np.array([[float(adet * v) for v in row] for row in t["M"]])
            assert np.abs(M - e[f"mass_p{order}_{nm}"]).max() <= 1e-13 * np.abs(M).max()
            for lf in range(4):
                s = hp.facet_scale(e[nm], lf)
                F = np.array([[float(s * v) for v in row] for row in t["F"][lf]])
                assert np.abs(F - e[f"facet_mass{lf}_p{order}_{nm}"]).max() <= 1e-13 * max(np.abs(F).max(), 1e-300)


def test_metric_asks_for_the_bits_where_the_scale_is_zero():
    ref = np.array([1.0, 0.0, 2.0])
    assert hp.metric(np.array([1.0, 0.0, 2.0 + 2.0 ** -51]), ref, np.array([0.0, 0.0, 1.0])) == 2.0 ** -51
    with pytest.raises(AssertionError):
        hp.metric(np.array([1.0, 1e-300, 2.0]), ref, np.array([0.0, 0.0, 1.0]))
    assert hp.metric(ref, ref, np.zeros(3)) == 0.0


def test_assembled_reference_is_the_sum_of_its_cells():
    """matrix(), vector(), dirichlet(), diagonal() and apply() on a mesh of a few cells against the dense sums"""
    C = _hostile.case("rotated", 2)
    keep = np.arange(12)
    cells, cd = C.cells[keep], C.cell_dofs[keep]
    n = C.n
    D = [[hp.mp.mpf(0)] * n for _ in range(n)]
    Ds = np.zeros((n, n))
    for c in range(len(keep)):
        A, sc = hp.element_matrix(2, C.x[cells[c]])
        for i in range(10):
            for j in range(10):
                D[cd[c, i]][cd[c, j]] += A[i][j]
                Ds[cd[c, i], cd[c, j]] += sc[i, j]
    rp, cl = zo.pattern(n, cd, 1)
    R, S = hp.matrix(2, C.x, cells, cd, rp, cl)
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.testing.assert_array_equal(R, np.array([float(D[i][j]) for i, j in zip(rows, cl)]))
    np.testing.assert_allclose(S, Ds[rows, cl], rtol=1e-14, atol=0)
    assert np.all(S[np.abs(R) > 0] > 0)
    Rc, Sc = hp.dirichlet(R, S, rp, cl, C.bc)
    b = C.bc.astype(bool)
    k = b[rows] | b[cl]
    assert np.all(Rc[k & (rows != cl)] == 0) and np.all(Rc[k & (rows == cl)] == 1) and np.all(Sc[k] == 0)
    np.testing.assert_array_equal(Rc[~k], R[~k])
    touched = np.diff(rp) > 0
    if touched.all():
        d, _ = hp.diagonal(R, S, rp, cl)
        np.testing.assert_array_equal(d, np.array([float(D[i][i]) for i in range(n)]))
    u = np.random.default_rng(3).standard_normal(n)
    rp2, cl2 = C.rowptr, C.cols
    Rf, Sf = hp.matrix(2, C.x, C.cells[:40], C.cell_dofs[:40], rp2, cl2)
    y, t = hp.apply(Rf, Sf, rp2, cl2, u)
    import scipy.sparse as sp
    yd = sp.csr_matrix((Rf, cl2, rp2), shape=(n, n)) @ u
    assert np.abs(y - yd).max() <= 8 * hp.U * t.max() and np.all(t >= np.abs(y))


ORACLE_FIGURES = [("identity", 1, 1.8), ("offset", 1, 1.8), ("aniso", 1, 1.8), ("graded", 1, 1.8), ("rotated", 1, 1.8),
                  ("needle", 1, 1.8), ("noise13", 1, 1.8), ("aniso", 2, 2.2), ("graded", 3, 5.9),
                  ("shear50_a", 1, 23.6), ("shear50_a", 2, 26.3), ("shear50_a", 3, 24.9)]


@pytest.mark.parametrize("name,order,measured", ORACLE_FIGURES, ids=[f"{n}-P{o}" for n, o, _ in ORACLE_FIGURES])
def test_oracle_figures_on_the_hostile_meshes(name, order, measured):
    C = _hostile.case(name, order)
    assert C.dims == _hostile.BASE[order]
    R, S = hp.matrix(order, C.x, C.cells, C.cell_dofs, C.rowptr, C.cols)
    ou = zo.assemble_matrix(0, order, C.x, C.cells, C.cell_dofs, np.zeros_like(C.bc), C.rowptr, C.cols)
    fig = hp.metric(ou, R, S) / hp.U
    print(f"oracle against the 50-digit reference, {name} P{order}: {fig:.2f} x 2^-53 (measured {measured})")
    assert np.all(S > 0)
    assert fig <= 2 * measured
