"""KSPPIPECG restated in plain numpy (Ghysels & Vanroose, Parallel Computing 40 (2014), Alg. 4; left-preconditioned, zero
initial guess): the yardstick of tests/test_pipecg_ref.py (CPU) and tests/test_gpu_pipecg.py.  It follows the listing
literally -- u and q by their recurrences, products through zo.spmv -- and shares no code with the library.  The
keyword arguments exist to MEASURE what rounding alone does to the iteration count: `dot` replaces the summation order
of the three sums, `recompute` forms u = D^-1 r and q = D^-1 s afresh instead of by recurrence (what the GPU kernel does)."""
import numpy as np
import zzz_oracle as zo

CASES = [("poisson", 1, (12, 10, 14)), ("poisson", 2, (6, 5, 7)), ("poisson", 3, (4, 3, 5)), ("elasticity", 1, (6, 6, 6)),
         ("elasticity", 2, (3, 3, 4))]  # the five of test_single_reduction_cg
# The spread of the restatement's iteration count under rounding alone, measured by tests/test_pipecg_ref.py on these
# fifteen (case, norm) pairs at rtol 1e-9 in four variants (sums plain / in reversed chunks of 64, u and q by recurrence /
# recomputed): 0 in thirteen pairs, 1 in two (Poisson P3 unpreconditioned: 117 117 116 117; elasticity P2 natural:
# 201 201 200 201).  The GPU bar on the count is this spread + 2, the + 2 being the standing allowance of the other forms.
MEASURED_SPREAD = 1
IT_BAR = MEASURED_SPREAD + 2
NORMS = [zo.NORM_PRECONDITIONED, zo.NORM_UNPRECONDITIONED, zo.NORM_NATURAL]


def dot_chunks_reversed(a, b, chunk=64):
    """<a,b> summed in chunks of 64, the chunks taken last to first"""
    s = 0.0
    for lo in range(((a.size - 1) // chunk) * chunk, -1, -chunk):
        s += float(np.dot(a[lo:lo + chunk], b[lo:lo + chunk]))
    return s


def diagonal(rowptr, cols, vals):
    n = rowptr.shape[0] - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    d = np.zeros(n)
    on = cols == rows
    d[rows[on]] = vals[on]
    d[d == 0.0] = 1.0  # PCJACOBI replaces zero diagonal entries by one
    return d


def pipecg_ref(rowptr, cols, vals, b, pc, norm_type, rtol, atol=1e-50, max_it=10000, dtol=1e4, dot=np.dot, recompute=False):
    """returns (iterations, x, final norm, initial norm, history)"""
    rowptr = rowptr.astype(np.int64)
    A = lambda v: zo.spmv(rowptr, cols, vals, np.ascontiguousarray(v))  # noqa: E731
    dinv = 1.0 / diagonal(rowptr, cols, vals) if pc == zo.PC_JACOBI else np.ones_like(b)
    x = np.zeros_like(b)
    r = b.copy()
    u = dinv * r
    w = A(u)
    z = q = p = s = None
    gamma_old = alpha_old = dp0 = ttol = None
    hist = []
    for i in range(max_it + 1):
        gamma, delta = float(dot(r, u)), float(dot(w, u))
        if norm_type == zo.NORM_NATURAL:
            dp = np.sqrt(abs(gamma))
        else:
            dp = np.sqrt(float(dot(r, r) if norm_type == zo.NORM_UNPRECONDITIONED else dot(u, u)))
        m = dinv * w
        n = A(m)
        hist.append(dp)
        if i == 0:
            dp0, ttol = dp, max(rtol * dp, atol)
        if not np.isfinite(dp) or dp <= ttol or dp >= dtol * dp0 or i == max_it:
            return i, x, dp, dp0, np.array(hist)
        if i == 0:
            alpha = gamma / delta
            z, q, p, s = n.copy(), m.copy(), u.copy(), w.copy()
        else:
            beta = gamma / gamma_old
            alpha = gamma / (delta - beta * gamma / alpha_old)
            z, q, p, s = n + beta * z, m + beta * q, u + beta * p, w + beta * s
        if recompute:
            q = dinv * s
        x = x + alpha * p
        r = r - alpha * s
        u = dinv * r if recompute else u - alpha * q
        w = w - alpha * z
        gamma_old, alpha_old = gamma, alpha
