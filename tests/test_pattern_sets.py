"""The claims of tests/_pattern_sets.py, proven without a GPU: every limit case sits exactly on its limit and its twin
exactly one unit past it, by counts made a second time with plain Python sets; the limits are the ones the sources have;
the oracle's pattern on these meshes is the brute-force one; the fan keeps its shape at every k; and the paths the claims
predict cover every value of the report (zzz_pattern_info) -- so that a case dropped from the table is noticed here."""
import os
import re

import numpy as np
import pytest

import _pattern_sets as ps
import zzz_oracle as zo

CSRC = os.path.join(ps.ROOT, "performance-test_amd", "csrc")


def _recount(c):
    """the branching quantities once more, cell by cell, with no numpy in the counting"""
    cd = c.cell_dofs.tolist()
    nd, n = len(cd[0]), c.n_owned
    rows = [set() for _ in range(n)]
    val = [0] * n
    nwin = (n + 255) // 256
    win = [0] * nwin
    for dofs in cd:
        for d in dofs:
            if d // 256 < nwin:
                win[d // 256] += 1
            if d < n:
                val[d] += 1
                rows[d].update(dofs)
    cut_cells, records = 0, 0
    for a, b in zip(cd[:-1], cd[1:]):
        k = sum(1 for u, v in zip(a, b) if v <= u)
        records += k
        cut_cells += 1 if k else 0
    blk = [sum(val[i:i + 128]) for i in range(0, n, 128)]
    return dict(nd=nd, blocks=cut_cells + 1, break_records=records, runs=(cut_cells + 1) * nd, window_max=max(win),
                block_adj_max=max(blk), cand_max=max(val) * nd, cols_max=max(len(r) for r in rows)), rows


def test_the_limits_are_the_ones_in_the_sources():
    pat = open(os.path.join(CSRC, "zzz_pattern.hip")).read()
    asm = open(os.path.join(CSRC, "zzz_assemble.hip")).read()
    internal = open(os.path.join(CSRC, "zzz_internal.h")).read()

    def const(src, name):
        m = re.search(r"constexpr int(?:[^;]*?[ ,])?" + name + r" = (\d+)", src)
        assert m, name
        return int(m.group(1))

    assert const(pat, "ADJ_W") == ps.ADJ_W and const(pat, "ADJ_CAP") == ps.ADJ_CAP
    assert const(pat, "ADJ_MAX_RUNS") == ps.ADJ_MAX_RUNS and const(pat, "ADJ_BREAK_CAP") == ps.ADJ_BREAK_CAP
    assert const(pat, "PAT_CAP") == ps.PAT_CAP and const(pat, "ROW_T_BLOCK") == ps.ROW_T_BLOCK
    for cap in ps.ROW_T_CAPS:
        assert f"k_row_pattern_thread4<{cap}, {ps.ROW_T_ADJ}>" in pat
    assert "for (int cap = 16; cap <= 32; cap *= 2)" in pat
    for cap in ps.REG_CAPS:
        assert f"ZZZ_ROW_REGS({cap});" in pat
    assert "if (P <= 512)" in pat and "if (n > PAT_CAP)" in pat
    assert const(internal, "SPMV_TILE_NNZ") == ps.SPMV_TILE_NNZ
    assert const(asm, "ASM_NNZ_P1") == ps.ASM_TILE_NNZ[(1, 1)] and const(asm, "ASM_NNZ_NODE3") == ps.ASM_TILE_NNZ[(1, 3)]
    assert "const int64_t Ws = (int64_t)SPMV_TILE_NNZ - maxrow - 2;" in pat
    assert "if (Ws < maxrow || Wa < maxblock || Wa < 1)" in pat
    assert ps.tile_limit(1, 1) == 960 and ps.tile_limit(1, 3) == 341


@pytest.mark.parametrize("name", ps.NAMES)
def test_claim_by_a_second_count(name):
    c = ps.case(name)
    mine, rows = _recount(c)
    assert mine == c.claim
    if c.limit:
        assert mine[c.limit[0]] == c.limit[1]
    # the oracle's pattern is the brute-force one
    rp, cl = zo.pattern(c.n_owned, c.cell_dofs, c.bs)
    bs = c.bs
    want = [[col * bs + d for col in sorted(r) for d in range(bs)] for r in rows for _ in range(bs)]
    assert rp.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert cl.tolist() == [v for w in want for v in w]
    # a mesh the library can take: every cell has four distinct vertices and nd distinct dofs, inside the ranges
    assert all(len(set(v)) == 4 for v in c.cells.tolist()) and all(len(set(v)) == mine["nd"] for v in c.cell_dofs.tolist())
    assert 0 <= c.cell_dofs.min() and c.cell_dofs.max() < c.n_owned + c.n_ghost and c.cells.max() < c.x.shape[0]
    assert c.facets.shape[0] == 0 or (c.facets[:, 0].max() < c.cells.shape[0] and c.facets[:, 1].max() < 4)


@pytest.mark.parametrize("at,past,quantity,unit", ps.PAIRS, ids=[p[0] for p in ps.PAIRS])
def test_limit_and_twin(at, past, quantity, unit):
    """the limit case has its maximum ON the capacity (the largest multiple of the unit -- one cell's candidates, one block's
    runs -- that fits) and nothing above; the twin is exactly one unit above"""
    a, b = _recount(ps.case(at))[0][quantity], _recount(ps.case(past))[0][quantity]
    caps = [cap for cap in ps.CAPACITY[quantity] if cap // unit * unit == a]
    assert len(caps) == 1, (a, ps.CAPACITY[quantity])
    assert b == a + unit and b > caps[0]
    # and the two differ in nothing else that decides a path, unless the path says so: same order, same problem
    assert (ps.case(at).order, ps.case(at).bs) == (ps.case(past).order, ps.case(past).bs)


def test_every_capacity_has_its_pair():
    seen = {q: set() for q in ps.CAPACITY}
    for at, _, q, unit in ps.PAIRS:
        v = ps.case(at).claim[q]
        seen[q].update(cap for cap in ps.CAPACITY[q] if cap // unit * unit == v)
    assert seen == {q: set(v) for q, v in ps.CAPACITY.items()}
    # candidates: every sort size at P1 (fans), P2 and P3 (repeats)
    for order, unit in ((1, 4), (2, 10), (3, 20)):
        got = {cap for at, _, q, u in ps.PAIRS if q == "cand_max" and ps.case(at).order == order
               for cap in ps.CAPACITY[q] if cap // u * u == ps.case(at).claim[q]}
        assert got == set(ps.CAPACITY["cand_max"]), (order, got)
    assert all(n in ps.TABLE for p in ps.PAIRS for n in p[:2])


def test_fan_shape():
    """|det J| = r_i r_(i+1) sin THETA with radii in [1, 1.5): no cell of any fan in the table is worse than 0.4 of the best"""
    ks = sorted({ps.case(n).cells.shape[0] for n in ps.NAMES if n.startswith("fan")})
    assert ks[0] == 13 and ks[-1] == 958
    for k in ks:
        x, cells = ps.fan_mesh(k)
        assert np.unique(x, axis=0).shape[0] == k + 3
        assert ps.fan_shape(k) >= ps.FAN_SHAPE_BOUND, k
        d = np.linalg.det(x[cells][:, 1:] - x[cells][:, :1])
        r = np.hypot(x[2:, 0], x[2:, 1])
        np.testing.assert_allclose(np.abs(d), r[:-1] * r[1:] * np.sin(ps.THETA), rtol=1e-12)


def test_the_claimed_paths_cover_the_report():
    """every value of the adjacency, row-kernel and builder fields, and every sort of the wavefront kernel, is predicted for
    some case (builder 2, ZZZ_PATTERN=host, is every case's own second run in tests/test_gpu_pattern_edges.py)"""
    adjacency, row_kernel, builder, sort = ps.covered_paths()
    assert adjacency == {0, 1, 2, 3}
    assert row_kernel == {-1, 0, 16, 32}
    assert builder == {0, 1}
    assert sort == {0, 64, 128, 256, 512, 1024}
    paths = [ps.case(n).path for n in ps.NAMES]
    assert {p["have_asm_pos"] for p in paths} == {0, 1} and {p["adj_source"] for p in paths} == {0, 1}
    assert sum(p["refused"] for p in paths) == 2
    # positions refused by a row of 513 .. 1024 candidates (pos_missed), at P2 and P3
    for order in (2, 3):
        assert any(ps.case(n).order == order and 512 < ps.case(n).claim["cand_max"] <= 1024 and not ps.case(n).path["have_asm_pos"]
                   for n in ps.NAMES)
    # the wavefront kernel at P1 for each of its two reasons: a row of more than 32 columns; a block past ROW_T_ADJ alone
    assert ps.case("fan_30").path["row_kernel"] == 0 and ps.case("block_adj_4097").claim["cols_max"] <= 16
    assert ps.case("block_adj_4097").path["row_kernel"] == 0 and ps.case("block_adj_4096").path["row_kernel"] == 16
    assert ps.case("window_7169").path["adjacency"] == 3 and ps.case("window_7168").path["adjacency"] == 1
    assert ps.case("p2_window_7169").path["adjacency"] == 3 and ps.case("p2_window_7168").path["adjacency"] == 1
    c = ps.case("p2_window_7169_then_host")
    assert c.claim["runs"] <= ps.ADJ_MAX_RUNS and c.claim["cand_max"] > ps.PAT_CAP and c.path["builder"] == 1
    assert ps.case("p1_blocks_128").path["adjacency"] == 1 and ps.case("p1_blocks_129").path["adjacency"] == 2
    assert ps.case("p2_blocks_51").path["adjacency"] == 1 and ps.case("p2_blocks_52").path["adjacency"] == 2
