"""The shared scratch of the set-up's device primitives (csrc/zzz_prim.h) across problems of different sizes on ONE context:
small, larger (the scratch grows: the old buffer is retired), small again (the buffer is now too large, and kept).  What every
step builds must be, byte for byte, what a fresh context builds for the same problem."""
import numpy as np
import pytest
import zzz

pytestmark = pytest.mark.gpu


def _build(c, problem, order, dims, block_rows):
    """CSR, right-hand side and one product of the cube problem, generated, patterned and assembled on context c"""
    form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
    c.cube_generate(problem, order, *dims)
    c.pattern_build()
    c.assemble_matrix(form)
    c.assemble_vector(form)
    rowptr, cols, vals = c.csr_download()
    b = c.vec_download(zzz.VEC_B)
    # (the product packs its form of the matrix if the assembly has not: the packers' scans run on the same scratch)
    y = c.spmv(np.random.default_rng(7).standard_normal(rowptr.shape[0] - 1))
    assert bool(c.spmv_values_info()["block_rows"]) == block_rows
    return {"rowptr": rowptr, "cols": cols, "vals": vals, "b": b, "y": y}


@pytest.mark.parametrize("problem,order,sequence,knobs", [
    ("poisson", 1, [(4, 4, 4), (12, 12, 12), (4, 4, 4)], {}),
    # the block-row packer's scan: the form is taken below its size rule too (knobs read when a context is created)
    ("elasticity", 2, [(3, 3, 3), (6, 6, 6)], {"ZZZ_SELLP_BLK": "2", "ZZZ_SELLP": "2"}),
])
def test_live_context_builds_what_a_fresh_one_builds(monkeypatch, problem, order, sequence, knobs):
    assert zzz.device_count() >= 1, "no GPU visible: these tests must not pass on a fallback"
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    fresh = {}
    for dims in set(sequence):
        with zzz.Context(0) as c:
            fresh[dims] = _build(c, problem, order, dims, bool(knobs))
    with zzz.Context(0) as live:
        for step, dims in enumerate(sequence):
            got = _build(live, problem, order, dims, bool(knobs))
            for name, want in fresh[dims].items():
                assert got[name].dtype == want.dtype and got[name].shape == want.shape, (step, dims, name)
                assert got[name].tobytes() == want.tobytes(), (step, dims, name)
