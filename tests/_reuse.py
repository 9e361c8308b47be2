"""States, feeds and the observation of tests/test_gpu_context_reuse.py: one context used for several problems in a row must
compute, byte for byte, what a fresh context computes for the last of them.

A State is one complete problem and the route by which a context is given it (uploaded arrays, or zzz_cube_generate).
observe(c, S) takes everything the ABI serves for that state -- orders, CSR, the right-hand sides, products, actions, every
solve form, the multigrid hierarchies -- into an ordered dict of numpy arrays; differing(a, b) names the entries whose bytes,
dtype or shape differ.  The knobs below make the special forms (operator stream, block rows, block windows, coded inverse
diagonal, deferred solution update) serve at these small sizes; observe asserts that they did, so that no comparison passes
because a cache was never built."""
import os
import types
from collections import OrderedDict

import numpy as np
import zzz
import zzz_oracle as zo

# read when a context is created: set (monkeypatch) before the first one, fresh and live contexts then see the same
KNOBS = {"ZZZ_SELLP": "2", "ZZZ_SELLP_BLK": "2", "ZZZ_SELLP_BWIN": "2", "ZZZ_CG_DINV_CODES": "2", "ZZZ_CG_XDEFER": "2"}
DICT_KNOB = {"ZZZ_SELLP_DICT": "2"}  # on top of KNOBS, in the tests of the stream's value dictionary alone
MAX_IT, RTOL = 25, 1e-10  # only the iterates matter, not convergence
COARSE_LIMIT = 20         # pc_mg_coarse_eq_limit: every hierarchy below has at least two levels (asserted)


class State:
    """name; route 'uploaded' | 'generated' | 'non-lattice'; P: the arrays (a zzz.Part or a namespace with its fields);
    dims: the cube of a generated state"""

    def __init__(self, name, route, P, dims=None):
        self.name, self.route, self.P, self.dims = name, route, P, dims
        self.problem = "elasticity" if P.bs == 3 else "poisson"
        self.order, self.bs, self.form = P.order, P.bs, P.form
        self.n = P.n_owned * P.bs
        self.mg = route == "generated"  # ZZZ_PC_MG / ZZZ_PC_PMG serve a generated cube only

    def feed(self, c):
        if self.route == "generated":
            c.cube_generate(self.problem, self.order, *self.dims)
        else:
            c.upload_part(self.P)

    def feed_behind_mesh(self, c):
        """everything upload_part uploads after the mesh: the dofmap and what hangs on it"""
        P = self.P
        c.upload_dofmap(P.order, P.bs, P.cell_dofs, P.n_owned, P.n_ghost)
        self.feed_behind_dofmap(c)

    def feed_behind_dofmap(self, c):
        P = self.P
        c.upload_bc(P.bc_dofs)
        c.upload_facets(P.facets)
        c.upload_coeff(zzz.COEFF_F, P.f)
        if P.g is not None:
            c.upload_coeff(zzz.COEFF_G, P.g)

    def bc_marker(self):
        m = np.zeros(self.n, np.uint8)
        m[self.P.bc_dofs] = 1
        return m

    def but(self, name, **changes):
        """the same state with some arrays replaced"""
        Q = types.SimpleNamespace(**{k: getattr(self.P, k) for k in _FIELDS})
        for k, v in changes.items():
            setattr(Q, k, v)
        return State(name, self.route, Q, self.dims)


_FIELDS = ("order", "bs", "form", "x", "cells", "cell_dofs", "n_owned", "n_ghost", "bc_dofs", "facets", "f", "g")


def _namespace(**kw):
    assert set(kw) == set(_FIELDS)
    return types.SimpleNamespace(**kw)


def _jittered():
    """the jittered, sheared, shuffled non-lattice mesh of test_unsorted_cells_and_foreign_numbering, P1 Poisson"""
    O = zo.Problem("poisson", 1, 3, 2, 3)
    rng = np.random.default_rng(12)
    perm = rng.permutation(O.cells.shape[0])
    cells = np.ascontiguousarray(O.cells[perm])
    cell_dofs = np.ascontiguousarray(O.cell_dofs[perm])
    M = np.array([[1.3, 0.2, 0.0], [0.1, 0.9, 0.3], [0.0, -0.2, 1.1]])
    jitter = 0.06 * (rng.random(O.x.shape) - 0.5)
    x = np.ascontiguousarray((O.x + jitter) @ M.T + np.array([0.3, -0.1, 0.2]))
    return _namespace(order=1, bs=1, form=zzz.FORM_POISSON, x=x, cells=cells, cell_dofs=cell_dofs, n_owned=O.nblock, n_ghost=0,
                      bc_dofs=np.nonzero(O.bc)[0].astype(np.int32), facets=zo.exterior_facets(cells), f=O.f, g=O.g)


def _generated(problem, order, dims):
    # zzz_cube_generate is "equivalent to uploading the arrays of zzzh_part_create": those arrays are the oracle's inputs
    return zzz.Part(problem, order, *dims)


_BUILDERS = OrderedDict([
    ("U1", lambda: State("U1", "uploaded", zzz.Part("poisson", 1, 5, 4, 6))),
    ("U1r", lambda: State("U1r", "uploaded", zzz.Part("poisson", 1, 5, 4, 6).renumbered("random"))),
    ("U1big", lambda: State("U1big", "uploaded", zzz.Part("poisson", 1, 12, 12, 12))),
    ("U2r", lambda: State("U2r", "uploaded", zzz.Part("poisson", 2, 3, 3, 4).renumbered("random"))),
    ("U3", lambda: State("U3", "uploaded", zzz.Part("poisson", 3, 2, 3, 2))),
    ("E1r", lambda: State("E1r", "uploaded", zzz.Part("elasticity", 1, 4, 4, 4).renumbered("random"))),
    ("E2", lambda: State("E2", "uploaded", zzz.Part("elasticity", 2, 3, 3, 3))),
    ("J", lambda: State("J", "non-lattice", _jittered())),
    ("G1", lambda: State("G1", "generated", _generated("poisson", 1, (6, 5, 4)), (6, 5, 4))),
    ("G2", lambda: State("G2", "generated", _generated("poisson", 2, (4, 3, 3)), (4, 3, 3))),
    ("GE1", lambda: State("GE1", "generated", _generated("elasticity", 1, (4, 4, 4)), (4, 4, 4))),
    # (not in the issue's table, which has no generated P3 cube: ZZZ_PC_PMG at order 3 needs one)
    ("G3", lambda: State("G3", "generated", _generated("poisson", 3, (2, 3, 2)), (2, 3, 2))),
])
NAMES = list(_BUILDERS)
_states = {}


def state(name):
    if name not in _states:
        _states[name] = _BUILDERS[name]()
    return _states[name]


def p1_on_mesh_of(S, name):
    """The P1 Poisson problem on the mesh of state S (any order), numbered as S numbers its vertices: dof i is vertex i.  With
    S's own dofmap uploaded behind it, that is 'a second dofmap on the same mesh'."""
    P = S.P
    dims = state_dims(S)
    R = zzz.Part("poisson", 1, *dims)  # the structured P1 problem: its dofs are its vertices
    assert np.array_equal(R.cells, R.cell_dofs) and R.n_owned == P.x.shape[0]
    # vertex of the structured mesh -> vertex of S's numbering, by coordinates
    key = lambda x: np.lexsort(np.round(x * 4096).astype(np.int64).T)  # (lattice coordinates: multiples of 1/n, far apart)
    new_of_old = np.empty(R.nverts, np.int64)
    new_of_old[key(R.x)] = key(P.x)
    assert np.array_equal(P.x[new_of_old], R.x)
    f, g = np.empty_like(R.f), np.empty_like(R.g)
    f[new_of_old], g[new_of_old] = R.f, R.g
    return State(name, S.route, _namespace(order=1, bs=1, form=zzz.FORM_POISSON, x=P.x, cells=P.cells, cell_dofs=P.cells.copy(),
                                           n_owned=R.n_owned, n_ghost=0, bc_dofs=np.sort(new_of_old[R.bc_dofs]).astype(np.int32),
                                           facets=zo.exterior_facets(P.cells), f=f, g=g), S.dims)


def state_dims(S):
    return S.dims if S.dims is not None else S.P.dims


def scalar_on_dofmap_of(S, name):
    """A Poisson problem (block size 1) on the mesh AND the block dofmap of the elasticity state S: the same dofmap uploaded at
    another block size.  Its Dirichlet set, f and g are taken from S's arrays (any values serve)."""
    P = S.P
    assert P.bs == 3
    return State(name, S.route, _namespace(order=P.order, bs=1, form=zzz.FORM_POISSON, x=P.x, cells=P.cells, cell_dofs=P.cell_dofs,
                                           n_owned=P.n_owned, n_ghost=0, bc_dofs=np.unique(P.bc_dofs // 3).astype(np.int32),
                                           facets=zo.exterior_facets(P.cells), f=np.ascontiguousarray(P.f[0::3]),
                                           g=np.ascontiguousarray(P.f[1::3]) * 1e-3), S.dims)


# ---- the observation ------------------------------------------------------------------------------------------------------
def _ints(d):
    return np.array([int(v) for v in d.values()], np.int64)


def _solve(c, S, out, tag, f32=False, **kw):
    c.vec_upload(zzz.VEC_U, np.zeros(S.n))  # (ZZZ_CG_CGH and the float solve start from u)
    solve = c.cg_solve_f32 if f32 else c.cg_solve
    it, rn, r0 = solve(rtol=RTOL, max_it=MAX_IT, **kw)
    info = c.cg_info()
    out[tag + ".iterations"] = np.int64(it)
    out[tag + ".rnorm"] = np.array([rn, r0])
    out[tag + ".history"] = c.cg_history(it + 1)
    out[tag + ".u"] = c.vec_download(zzz.VEC_U)
    out[tag + ".reason"] = np.int64(c.cg_reason())
    out[tag + ".info"] = np.array([float(v) for v in info.values()])
    return info


def _hierarchy(c, out, tag, level_csr):
    top = c.mg_info()
    assert top["levels"] >= 2, (tag, top)
    out[tag + ".mg_info"] = np.array([top[k] for k in ("levels", "coarse_dofs", "products_per_cycle", "high_order_levels")], np.int64)
    for l in range(top["levels"]):
        li = c.mg_info(l)
        out[f"{tag}.mg_info{l}"] = np.array(list(li["cells"]) + [li["dofs"], li["nnz"], li["hi"], li["lo"], li["degree"]], np.float64)
    if level_csr:
        for k, a in zip(("rowptr", "cols", "vals"), c.mg_level_csr(1)):
            out[f"{tag}.level1.{k}"] = a


def vectors(n):
    """the observation's fixed inputs: x of the products and actions; u0, the non-zero Dirichlet values"""
    rng = np.random.default_rng(5)
    return rng.standard_normal(n), 0.5 + rng.random(n)


def observe(c, S, matrix="assembled"):
    """Everything the ABI serves for state S on context c, which has been fed S.  matrix = 'assembled': pattern build and
    matrix assembly are part of the observation; 'reassembled': the matrix is assembled on the pattern the context already
    has, with NO pattern build (a pattern build alone drops the stream, the lifting rows and the agg hierarchy: the caches
    that hang on the Dirichlet set or on the values are then never the thing under test); 'kept': the context's pattern and
    values are taken as they stand (after zzz_csr_upload_values)."""
    out = OrderedDict()
    form, n = S.form, S.n
    x, u0 = vectors(n)
    perm, kind = c.internal_order()
    out["perm"], out["kind"], out["cells_renumbered"] = perm, np.int64(kind), np.int64(c.cells_renumbered())
    assert matrix in ("assembled", "reassembled", "kept")
    if matrix == "assembled":
        c.pattern_build()
    if matrix != "kept":
        c.assemble_matrix(form)
    out["rowptr"], out["cols"], out["vals"] = c.csr_download()
    c.assemble_vector(form)
    out["b"] = c.vec_download(zzz.VEC_B)
    c.upload_bc_values(u0)
    c.assemble_vector(form)
    out["b.lifted"] = c.vec_download(zzz.VEC_B)
    assert out["b.lifted"].tobytes() != out["b"].tobytes()
    c.upload_bc_values(None)
    c.assemble_vector(form)
    out["b.again"] = c.vec_download(zzz.VEC_B)
    # the product, on the forms the knobs select
    out["spmv"] = c.spmv(x)
    vi = c.spmv_values_info()
    out["spmv_values_info"] = np.array(c.spmv_values_info_raw(), np.int64)
    assert c.spmv_operator_form() == 1, "the product does not run on the operator stream"
    if S.bs == 3:
        assert vi["block_rows"], vi
    elif S.order > 1:
        assert vi["row_windows"], vi
    else:
        # P1 rows are short: the generic stream, whose values stay doubles at these sizes unless ZZZ_SELLP_DICT=2 (DICT_KNOB)
        # asks for the value dictionary -- then the one-chunk kernel on coded values with its packed palettes
        assert not vi["special_form"], vi
        if os.environ.get("ZZZ_SELLP_DICT") == "2":
            assert vi["form"] != "doubles" and vi["distinct_values"] > 1, vi
            if S.route != "non-lattice":
                assert vi["one_chunk_kernel"], vi
                # (uploaded values D A D leave 64 distinct codes in every slot: no slice is packed, and the palettes of the
                # assembled matrix must be gone)
                assert (vi["packed_slices"] > 0) == (matrix != "kept"), vi
    out["spmv_info"] = np.array(c.spmv_info_raw(), np.int64)
    # the matrix-free operator
    out["action"] = c.action(x)
    assert c.matfree_info()["valid"] == 1
    out["matfree_info"] = _ints(c.matfree_info())
    out["matfree_diagonal"] = c.matfree_diagonal()
    c.matfree_assemble_vector(form)
    out["b.matfree"] = c.vec_download(zzz.VEC_B)
    c.assemble_vector(form)  # (the solves below run on the pattern's right-hand side)
    if S.bs == 1:
        out["action_f32"] = c.action_f32(x.astype(np.float32))
        assert c.matfree_info_f32()["built"] == 1
        out["matfree_info_f32"] = _ints(c.matfree_info_f32())
        _solve(c, S, out, "cg_f32", f32=True)
    else:
        B, dev = c.near_nullspace()
        out["near_nullspace"], out["near_nullspace.deviation"] = B, np.float64(dev)
    # every solve form
    info = _solve(c, S, out, "jacobi", pc=zzz.PC_JACOBI)
    assert info["dinv_codes"] > 0 and info["xdefer_k"] > 1, info
    info = _solve(c, S, out, "jacobi_sr", pc=zzz.PC_JACOBI, single_reduction=True)
    assert info["dinv_codes"] > 0, info
    info = _solve(c, S, out, "pipe", variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI)
    assert info["dinv_codes"] > 0, info
    info = _solve(c, S, out, "none", pc=zzz.PC_NONE)
    assert info["xdefer_k"] > 1, info
    info = _solve(c, S, out, "chebyshev", pc=zzz.PC_CHEBYSHEV_JACOBI)
    assert info["pc_spectrum_bound"] > 0.0, info
    _solve(c, S, out, "cgh_matfree", variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE)
    _solve(c, S, out, "jacobi_matfree", pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE)
    if S.mg and matrix != "kept":
        pc, tag = (zzz.PC_MG, "mg") if S.order == 1 else (zzz.PC_PMG, "pmg")
        _solve(c, S, out, tag, pc=pc, pc_mg_coarse_eq_limit=COARSE_LIMIT)
        _hierarchy(c, out, tag, False)
        out[tag + ".apply"] = c.mg_apply(x)
    _solve(c, S, out, "agg", pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=COARSE_LIMIT)
    _hierarchy(c, out, "agg", True)
    out["agg.apply"] = c.mg_apply(x)
    return out


def differing(got, want, skip=()):
    """names of the observables whose bytes, dtype or shape differ (and of those only one side has)"""
    bad = [k for k in want if k not in got] + [k for k in got if k not in want]
    for k, w in want.items():
        if k in got and k not in skip:
            g = np.asarray(got[k])
            w = np.asarray(w)
            if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
                bad.append(k)
    return bad
