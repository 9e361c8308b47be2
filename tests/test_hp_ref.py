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

Elasticity, with the component-aware scale of _hp_ref.py, for the unconstrained matrix (the unconstrained vector in brackets;
P1 6x5x5 -- shear50_b 6x9x5 --, P2 3x3x4, P3 2x2x3 cubes; one thread):

    P1   identity 1.55 (4.52)   offset 2.20 (4.80)   aniso 2.34 (4.52)   needle 2.00 (4.52)   graded 2.93 (5.09)
         mirror 1.55 (4.77)   noise10 2.17 (4.57)   noise7 2.93 (4.69)   rotated 2.33 (3.96)
         shear50_a 26.15 (38.71)   shear50_b 22.83 (30.06)
    P2   aniso 3.61 (5.09)   graded 3.66 (4.75)   mirror 3.25 (4.28)   rotated 3.46 (4.28)   noise10 3.80 (4.15)
         shear50_a 25.91 (34.98)
    P3   offset 5.46 (9.52)   graded 6.37 (7.74)   rotated 5.48 (11.66)   shear50_a 33.70 (65.45)

Every scale of every case is > 0 (the smallest, on aniso, is 8.8e-20 of max|A| at P1 and 1.0e-20 at P2) and no figure comes
near 100, beyond which the GPU bar of 8 x the oracle's figure would mean nothing.  A handful are pinned below at twice the
measured figure; tests/test_gpu_hostile_elasticity.py takes every case.  (A rotated cube stretched by 2^10 and 2^-10 gives
4.6e7: a property of cond(J), not of any code, and not a case.)
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


@pytest.mark.parametrize("order", [1, 2, 3])
def test_elasticity_element_against_the_oracle(order):
    """Elasticity matrix and load of one cell (dofs 3 i + c) at the bar of the Poisson element test, every entry against its
    own component-aware scale; no entry of the full 3 nd x 3 nd block has scale 0"""
    nd = hp.tables(order)["nd"]
    rng = np.random.default_rng(200 + order)
    for xc in _tets(order):
        A, sc = hp.elasticity_element_matrix(order, xc)
        A = np.array([[float(v) for v in row] for row in A])
        assert np.all(sc > 0) and np.array_equal(A, A.T)
        assert hp.metric(zo.tabulate("elasticity_a", order, xc), A, sc) <= 64 * hp.U
        f = rng.standard_normal(3 * nd)
        b, s = hp.elasticity_element_vector(order, xc, f)
        assert np.all(s > 0)
        assert hp.metric(zo.tabulate("elasticity_L", order, xc, w=f), np.array([float(v) for v in b]), s) <= 64 * hp.U


def test_assembled_elasticity_reference_is_the_sum_of_its_cells():
    """elasticity_matrix() and elasticity_vector() on a mesh of a few cells against the dense sums of their cells"""
    C = _hostile.case("rotated", 2, "elasticity")
    cells, cd = C.cells[:6], C.cell_dofs[:6]
    n = C.n
    D = [[hp.mp.mpf(0)] * n for _ in range(n)]
    Ds = np.zeros((n, n))
    db, dbs = [hp.mp.mpf(0)] * n, np.zeros(n)
    for c in range(6):
        sd = (3 * cd[c][:, None] + np.arange(3)).reshape(-1)
        A, sc = hp.elasticity_element_matrix(2, C.x[cells[c]])
        be, bs = hp.elasticity_element_vector(2, C.x[cells[c]], C.f[sd])
        for i in range(30):
            db[sd[i]] += be[i]
            dbs[sd[i]] += bs[i]
            for j in range(30):
                D[sd[i]][sd[j]] += A[i][j]
                Ds[sd[i], sd[j]] += sc[i, j]
    rp, cl = zo.pattern(C.nblock, cd, 3)
    R, S = hp.elasticity_matrix(2, C.x, cells, cd, rp, cl)
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert len(cl) == np.count_nonzero(Ds)
    np.testing.assert_array_equal(R, np.array([float(D[i][j]) for i, j in zip(rows, cl)]))
    np.testing.assert_allclose(S, Ds[rows, cl], rtol=1e-14, atol=0)
    assert np.all(S > 0)
    r, s = hp.elasticity_vector(2, C.x, cells, cd, C.f, n)
    np.testing.assert_array_equal(r, np.array([float(v) for v in db]))
    np.testing.assert_allclose(s, dbs, rtol=1e-14, atol=0)


def test_dof_coordinates_of_a_mapped_case():
    """_hostile.dof_coords: on the unmapped cube it gives the oracle's dof coordinates, on a graded mesh the vertices sit at
    the mapped vertices and the other dofs do NOT sit at the map of their base coordinates"""
    for order in (2, 3):
        C = _hostile.case("identity", order, "elasticity")
        assert np.abs(_hostile.dof_coords(C) - C.dof_x_base).max() <= 4 * hp.U
        C = _hostile.case("graded", order, "elasticity")
        X = _hostile.dof_coords(C)
        np.testing.assert_array_equal(X[C.cell_dofs[:, :4]], C.x[C.cells])
        edge = np.setdiff1d(C.cell_dofs[:, 4:], C.cell_dofs[:, :4])
        assert np.abs(X[edge] - C.dof_x_base[edge] ** 3).max() > 1e-3


def test_elasticity_reference_annihilates_the_rigid_body_modes():
    """A pin that owes nothing to the oracle: the unconstrained reference matrix of `rotated` P2 applied to the three
    translations and the three rotations of the mapped dof coordinates.  Exactly, every row sums to zero against them; here
    the entries are rounded once (half a unit of their scale each: 0.5 of t) and the rotations carry the rounding of the dof
    coordinates (the affine image of a P2 node: a difference and a sum rounded, the product by 1/2 exact -- one unit of the
    coordinates, so 1 of t = sum_j S_ij |u_j|).  That is 1.5 units of apply()'s t at the worst; the bar is 2, and 0.05 to
    0.10 was measured.  A reference that lost a few digits in its own assembly, or swapped D_cd and D_dc, misses it."""
    C = _hostile.case("rotated", 2, "elasticity")
    ref = _hostile.reference(C)
    X = _hostile.dof_coords(C)
    one, zero = np.ones(C.nblock), np.zeros(C.nblock)
    modes = [(one, zero, zero), (zero, one, zero), (zero, zero, one),
             (-X[:, 1], X[:, 0], zero), (zero, -X[:, 2], X[:, 1]), (X[:, 2], zero, -X[:, 0])]
    for k, m in enumerate(modes):
        u = np.stack(m, axis=1).reshape(-1)
        y, t = hp.apply(ref["R"], ref["S"], C.rowptr, C.cols, u)
        fig = float((np.abs(y) / t).max()) / hp.U
        print(f"rigid-body mode {k}: |R u| / t = {fig:.2f} x 2^-53, |R u| / (|R| |u|) = {np.abs(y).max() / np.abs(ref['R']).max() / np.abs(u).max():.2e}")
        assert np.all(t > 0) and fig <= 2.0


ELASTICITY_ORACLE_FIGURES = [("identity", 1, 1.55), ("aniso", 1, 2.34), ("shear50_a", 1, 26.2), ("aniso", 2, 3.61),
                             ("rotated", 2, 3.46), ("offset", 3, 5.46)]


@pytest.mark.parametrize("name,order,measured", ELASTICITY_ORACLE_FIGURES, ids=[f"{n}-P{o}" for n, o, _ in ELASTICITY_ORACLE_FIGURES])
def test_oracle_figures_of_elasticity_on_the_hostile_meshes(name, order, measured):
    C = _hostile.case(name, order, "elasticity")
    assert C.dims == _hostile.ELASTICITY_BASE[order]
    ref = _hostile.reference(C)
    fig = ref["oracle_A_free"]
    print(f"oracle against the 50-digit reference, elasticity {name} P{order}: A {fig:.2f} x 2^-53 (measured {measured}),"
          f" b {ref['oracle_b_free']:.2f}")
    assert np.all(ref["S"] > 0) and np.all(ref["s_unc"] > 0)
    assert fig <= 2 * measured
    assert fig <= 100 and ref["oracle_b_free"] <= 100  # beyond that the GPU bar (8 x the oracle's figure) means nothing


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
