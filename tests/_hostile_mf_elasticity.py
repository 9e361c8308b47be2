"""The 50-digit reference of the matrix-free ELASTICITY action on the hostile meshes: TEST INFRASTRUCTURE ONLY.

tests/_hostile.py's action_reference is the Poisson one (its oracle figure comes from zo.action_poisson); this is the same
rule for block size 3: y = R u with products and sums in long double on the mp pass's unconstrained matrix, t its per-row
scale sum_j S_ij |u_j|, constrained rows y = 0 exactly with scale 0; the oracle's figure is that of its own unconstrained
matrix applied through zo.spmv with the constrained rows zeroed."""
import numpy as np

import _hostile as H
import _hp_ref as hp
import zzz_oracle as zo

CASES = [(n, o) for o in (1, 2, 3) for n in ("offset", "aniso", "graded", "rotated") if n in H.ELASTICITY_CASES[o]]


def action_reference(C, u):
    """(y, t, the oracle's figure in units of 2^-53)"""
    ref = H.reference(C)
    y, t = hp.apply(ref["R"], ref["S"], C.rowptr, C.cols, u)
    y, t = np.array(y, np.float64), np.array(t, np.float64)
    bcb = C.bc.astype(bool)
    y[bcb] = 0.0
    t[bcb] = 0.0
    oy = zo.spmv(np.ascontiguousarray(C.rowptr, np.int64), C.cols, ref["ou"], u)
    oy[bcb] = 0.0
    return y, t, hp.metric(oy, y, t) / hp.U
