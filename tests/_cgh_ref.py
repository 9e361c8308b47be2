"""linalg::cg (src/cg.h:38-86) restated in numpy on an assembled operator: TEST INFRASTRUCTURE ONLY.

The oracle has the matrix-free loop for the Poisson form alone (zo.cg_matfree_poisson); for elasticity the operator of
`cgelasticity` -- y = A_unconstrained x, then y[bc] = 0 -- is the oracle's unconstrained matrix applied through zo.spmv with the
constrained rows zeroed, and the loop below is the reference's, statement by statement."""
import numpy as np

import zzz_oracle as zo


def operator(rowptr, cols, vals_unconstrained, bc):
    """x -> A_unconstrained x with the rows of constrained scalar dofs set to 0"""
    free = ~np.asarray(bc).astype(bool)
    rp = np.ascontiguousarray(rowptr, np.int64)

    def action(x):
        return np.where(free, zo.spmv(rp, cols, vals_unconstrained, np.ascontiguousarray(x, np.float64)), 0.0)

    return action


def cg(action, b, x0=None, kmax=50, rtol=1e-8):
    """(k, x, history of <r, r> with the initial one first) of src/cg.h:38-86"""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    y = action(x)               # :46
    r = b - y                   # :47
    p = r.copy()                # :50
    rnorm0 = float(r @ r)       # :53
    rtol2 = rtol * rtol
    rnorm = rnorm0
    hist = [rnorm0]
    k = 0
    while k < kmax:             # :57
        k += 1
        y = action(p)           # :62
        alpha = rnorm / float(p @ y)
        x = x + alpha * p       # :68
        r = r - alpha * y       # :71
        rnorm_new = float(r @ r)
        beta = rnorm_new / rnorm
        rnorm = rnorm_new
        hist.append(rnorm)
        if rnorm / rnorm0 < rtol2:  # :78
            break
        p = beta * p + r        # :82
    return k, x, np.array(hist)
