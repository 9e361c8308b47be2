"""The numpy restatement of KSPPIPECG (tests/_pipecg_ref.py) pinned against the oracle's KSPCG on the project's own
matrices, before anything on the GPU is compared with it -- and the place where the margins of the GPU test are MEASURED:
the restatement's iteration count against classical CG's, and against itself under other roundings (the three sums in
reversed chunks of 64; u and q recomputed as D^-1 r, D^-1 s).  The figures are printed (pytest -s) and recorded in
DESIGN.md section 5a; the asserted spread is the one the GPU bar is built on."""
import numpy as np
import pytest
import zzz_oracle as zo
from _pipecg_ref import CASES, MEASURED_SPREAD, NORMS, dot_chunks_reversed, pipecg_ref

RTOL = 1e-9

_problems = {}


def problem(problem_type, order, dims):
    key = (problem_type, order, dims)
    if key not in _problems:
        zo.set_num_threads(1)
        _problems[key] = zo.Problem(problem_type, order, *dims).assemble()
    return _problems[key]


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("problem_type,order,dims", CASES)
def test_pipecg_ref_against_classical_cg(problem_type, order, dims, norm):
    P = problem(problem_type, order, dims)
    rp, cl, v, b = P.rowptr.astype(np.int64), P.cols, P.vals, P.b
    itc, uc, rnc, r0c = zo.pcg(rp, cl, v, b, pc=zo.PC_JACOBI, norm_type=norm, rtol=RTOL)
    it, u, rn, r0, hist = pipecg_ref(rp, cl, v, b, zo.PC_JACOBI, norm, RTOL)
    counts = {"plain": it}
    for name, kw in (("chunks", dict(dot=dot_chunks_reversed)), ("recompute", dict(recompute=True)),
                     ("chunks+recompute", dict(dot=dot_chunks_reversed, recompute=True))):
        counts[name] = pipecg_ref(rp, cl, v, b, zo.PC_JACOBI, norm, RTOL, **kw)[0]
    res = np.linalg.norm(b - zo.spmv(rp, cl, v, u)) / np.linalg.norm(b)
    print(f"pipecg_ref {problem_type} P{order} {dims} norm {norm}: classical {itc}, pipelined {counts}, "
          f"|u-uc|/|uc| {np.linalg.norm(u - uc) / np.linalg.norm(uc):.2e}, true residual {res:.2e}")
    assert abs(r0 - r0c) <= 1e-12 * r0c and rn <= RTOL * r0
    assert hist.shape[0] == it + 1 and hist[0] == r0 and hist[-1] == rn
    assert np.linalg.norm(u - uc) <= 1e-7 * np.linalg.norm(uc)
    assert res <= 1e-8
    assert abs(it - itc) <= 2  # the same iteration in exact arithmetic
    assert max(counts.values()) - min(counts.values()) <= MEASURED_SPREAD


@pytest.mark.parametrize("problem_type,order,dims", [CASES[0], CASES[3]])
def test_pipecg_ref_without_preconditioner_and_limits(problem_type, order, dims):
    P = problem(problem_type, order, dims)
    rp, cl, v, b = P.rowptr.astype(np.int64), P.cols, P.vals, P.b
    itc, uc, _, _ = zo.pcg(rp, cl, v, b, pc=zo.PC_NONE, rtol=RTOL)
    it, u, rn, r0, _ = pipecg_ref(rp, cl, v, b, zo.PC_NONE, zo.NORM_PRECONDITIONED, RTOL)
    assert abs(it - itc) <= 2 and np.linalg.norm(u - uc) <= 1e-7 * np.linalg.norm(uc)
    it, _, _, _, hist = pipecg_ref(rp, cl, v, b, zo.PC_JACOBI, zo.NORM_PRECONDITIONED, 1e-14, max_it=3)
    assert it == 3 and hist.shape[0] == 4
    it, u, rn, _, _ = pipecg_ref(rp, cl, v, np.zeros_like(b), zo.PC_JACOBI, zo.NORM_PRECONDITIONED, RTOL)
    assert it == 0 and rn == 0.0 and np.all(u == 0.0)
