"""What the GPU tests on the hostile meshes share (tests/test_gpu_hostile_geometry.py, tests/test_gpu_hostile_elasticity.py,
tests/test_gpu_f32_hostile.py): environment knobs, the upload of a case, the kind of internal order, the bar, one assembly
with its bit-for-bit checks.  TEST INFRASTRUCTURE ONLY."""
import contextlib
import os

import numpy as np

import _hostile as H
import zzz

MF_SMALL = dict(ZZZ_MF_T="128", ZZZ_MF_NC="128")  # even the P3 base (216 cells) then has a full and a partial block


@contextlib.contextmanager
def _env(**kw):
    """environment knobs for the block: a value of None means unset"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _upload(c, C, renumber):
    with _env(ZZZ_RENUMBER=renumber):
        c.upload_mesh(C.x, C.cells)
        c.upload_dofmap(C.order, C.bs, C.cell_dofs, C.nblock, 0)
    c.upload_bc(np.nonzero(C.bc)[0].astype(np.int32))
    c.upload_coeff(zzz.COEFF_F, C.f)
    if C.problem == "poisson":
        c.upload_facets(C.facets)
        c.upload_coeff(zzz.COEFF_G, C.g)


def _check_kind(c, C, renumber):
    """internal_order()[1] where the code fixes it.  Seen on the MI355X for the others (unset / ZZZ_RENUMBER=2):
    see the tables in the docstrings of the test modules."""
    kind = c.internal_order()[1]
    if C.name in H.KIND_LATTICE:
        assert kind == 1, (C.name, kind)
    elif C.name in H.KIND_CLOUD:
        assert kind == (2 if renumber == "2" else 0), (C.name, kind)
    else:
        assert kind in (0, 1, 2), (C.name, kind)
    return kind


def _bar(oracle_figure):
    return max(8.0 * oracle_figure, 32.0)


def _assembled(c, C):
    c.pattern_build()
    c.assemble_matrix(C.form)
    c.assemble_vector(C.form)
    rp, cl, v = c.csr_download()
    np.testing.assert_array_equal(rp, C.rowptr)
    np.testing.assert_array_equal(cl, C.cols)
    rp2, cl2, v2 = c.csr_download()
    np.testing.assert_array_equal(rp2, rp)
    np.testing.assert_array_equal(cl2, cl)
    np.testing.assert_array_equal(v2, v)
    b = c.vec_download(zzz.VEC_B)
    np.testing.assert_array_equal(c.vec_download(zzz.VEC_B), b)
    return rp, cl, v, b
