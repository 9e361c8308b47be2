"""ZZZ_PC_MG on several ranks, restated in numpy on tests/_mg_ref.py's P: level 0 lives on the z-slabs of zzz.Part(..., nparts,
rank), every coarser level is whole on every rank.  The rows of P~ cut at the parts' ownership are the owned prolongation; the
rank-ordered sum of the partial restrictions P~[rows of p].T r[rows of p] is the whole restriction up to rounding, within
test_gpu_mg's transfer bar (1e-13 of max |out|: a sum of at most about 30 terms, split in at most three places; 1.5e-16 is what the
shapes below give); and a part reaches only the coarse planes tc[p0] .. tc[p1] + 1 of its owned vertex planes [p0, p1] -- what the
slab restriction of csrc/zzz_mg.hip walks, the rest being zeroed."""
import numpy as np
import pytest
import scipy.sparse as sp
import zzz
from _mg_ref import level_dims, oracle_problem, prolongation

CASES = [("poisson", (10, 9, 12), 2), ("poisson", (10, 9, 12), 3), ("poisson", (10, 9, 12), 4), ("poisson", (7, 6, 9), 3),
         ("poisson", (6, 5, 3), 3), ("elasticity", (5, 5, 8), 2), ("elasticity", (5, 5, 8), 4)]
LIMIT = {(10, 9, 12): 200, (7, 6, 9): 100, (6, 5, 3): 50, (5, 5, 8): 200}


def _masked_p(kind, n, nc, bs):
    free = [sp.diags(1.0 - oracle_problem(kind, d).bc.astype(float)) for d in (n, nc)]
    return (free[0] @ prolongation(n, nc, bs) @ free[1]).tocsr()


def test_the_level_tables_of_the_shapes():
    assert [np.prod([v + 1 for v in d]) for d in level_dims((10, 9, 12), 1, limit=200)] == [1430, 252, 64]
    for n, limit in LIMIT.items():
        assert len(level_dims(n, 3 if n == (5, 5, 8) else 1, limit=limit)) >= 2


@pytest.mark.parametrize("kind,n,nparts", CASES)
def test_slab_transfer_is_the_whole_transfer(kind, n, nparts):
    bs = 3 if kind == "elasticity" else 1
    nc = level_dims(n, bs, limit=LIMIT[n])[1]
    P = _masked_p(kind, n, nc, bs)
    rng = np.random.default_rng(5)
    e, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
    whole_pe, whole_rt = P @ e, P.T @ r
    plane, cplane = (n[0] + 1) * (n[1] + 1), (nc[0] + 1) * (nc[1] + 1)
    tc = [min(i * nc[2] // n[2], nc[2] - 1) for i in range(n[2] + 1)]
    total, offset, pieces = np.zeros(P.shape[1]), 0, []
    for rank in range(nparts):
        part = zzz.Part(kind, 1, *n, nparts, rank)
        lo, hi = part.own_offset * bs, (part.own_offset + part.n_owned) * bs
        assert lo == offset  # the parts own contiguous ranges, in rank order
        offset = hi
        # the owned vertex planes [p0, p1]: plane zs belongs to the part below (host/cube_layout.h)
        zs, ze = n[2] * rank // nparts, n[2] * (rank + 1) // nparts
        p0, p1 = (0 if rank == 0 else zs + 1), ze
        assert (lo, hi) == (p0 * plane * bs, (p1 + 1) * plane * bs)
        rows = P[lo:hi]
        pieces.append(rows @ e)
        partial = rows.T @ r[lo:hi]
        # the coarse planes this part reaches
        touched = np.unique(rows.tocoo().col // (cplane * bs))
        assert touched.min() >= tc[p0] and touched.max() <= tc[p1] + 1
        reach = np.zeros(P.shape[1], bool)
        reach[tc[p0] * cplane * bs:(tc[p1] + 2) * cplane * bs] = True
        assert not partial[~reach].any()
        total = total + partial  # rank order
    assert offset == P.shape[0]
    assert np.array_equal(np.concatenate(pieces), whole_pe)
    d = np.abs(total - whole_rt).max() / np.abs(whole_rt).max()
    print(f"slab restriction {kind} {n} on {nparts} parts: rank-ordered sum off by {d:.2e} of max |out|")
    assert d <= 1e-13
