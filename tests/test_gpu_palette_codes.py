"""GPU tests of the packed form of the one-chunk product's value codes (ZZZ_SELLP_PAL; csrc/zzz_sellp_dict.hip k_sp_pal_build,
csrc/zzz_sellp_pipe.hip spmv_one_kernel<..., PAL>): a slice none of whose eight slots holds more than 16 distinct codes is read
as 4-bit indices into per-slot palettes, 512 B for 1 024.

Values go in through csr_upload_values on a pattern assembled once; they come from tests/_palette_sets.py, and
tests/test_palette_value_sets.py proves on the CPU that every array holds the per-(slice, slot) counts its case claims.  The
stream dictionary and the one-chunk kernel are forced with the existing knobs (the default rules want larger matrices).

Bars: the product (plain, and the <x, A x> the dot form returns) against the oracle's serial CSR loop (zo.spmv) as BIT PATTERNS,
NaN exactly where the reference has it, with ZZZ_SELLP_PAL=1 and =0; solves with the knob 1 against 0: iterations, residual
histories and u identical bits (the arithmetic is the same, and a lane sums the same rows' terms: an affine pair keeps the pair
form whether its slices are packed or not); both against zo.pcg / zo.pcg_single_reduction with the project's bars (iterations
+-2, solution 1e-6).  Every case asserts the form it expects through spmv_values_info()."""
import contextlib

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
import _palette_sets as ps
from test_gpu_value_codes import _Env, _same_bits

pytestmark = pytest.mark.gpu

FORCED = dict(ZZZ_SELLP_DICT=2, ZZZ_SELLP=2)


@contextlib.contextmanager
def _context(name, pal):
    zo.set_num_threads(8)
    P, rp, cl, _ = ps.problem(name)
    with _Env(**FORCED):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("ZZZ_SELLP_PAL", str(pal))
            with zzz.Context(0) as c:
                c.upload_part(P)
                c.pattern_build()
                c.assemble_matrix(P.form)
                c.assemble_vector(P.form)
                crp, ccl, _ = c.csr_download(values=False)
                np.testing.assert_array_equal(crp, rp)
                np.testing.assert_array_equal(ccl, cl)
                yield c


_refs = {}


def _reference(case):
    """(x, the serial loop's product) of the case's values, computed once"""
    if case not in _refs:
        name = ps.CASES[case][0]
        _, rp, cl, _ = ps.problem(name)
        x = np.random.default_rng(41).standard_normal(rp.size - 1)
        with np.errstate(all="ignore"):
            _refs[case] = (x, zo.spmv(rp, cl, ps.values(case), x))
    return _refs[case]


def _product(c, case, pal):
    """upload the case's values; the product against the serial loop; returns spmv_values_info()"""
    x, ref = _reference(case)
    c.csr_upload_values(ps.values(case))
    y = c.spmv(x)
    vi = c.spmv_values_info()
    print(f"{case} PAL={pal}: packed {vi['packed_slices']} unpacked {vi['unpacked_slices']} mixed pairs {vi['mixed_pairs']} "
          f"largest slot {vi['max_codes_per_slot']} bytes {vi['bytes_per_product']}")
    assert vi["form"] == "dictionary in LDS" and vi["one_chunk_kernel"], vi
    _same_bits(y, ref, f"{case} PAL={pal}")
    if not pal:
        assert (vi["packed_slices"], vi["mixed_pairs"]) == (0, 0), vi
    return vi


def _slices(case):
    return (ps.problem(ps.CASES[case][0])[1].size - 1 + 63) // 64


@pytest.mark.parametrize("pal", [1, 0])
@pytest.mark.parametrize("case", ["assembled_p1_17", "assembled_p1_10_9_11"])
def test_assembled_values(case, pal):
    """the lattices' own matrices: some slices packed (the CPU count says which), the rest on their 16-bit codes, in one launch;
    the byte count is what the launched kernel addresses: 512 B less per packed slice"""
    with _context(ps.CASES[case][0], pal) as c:
        vi = _product(c, case, pal)
        raw = c.spmv_info_raw()
    assert vi["packed_slices"] + vi["unpacked_slices"] == _slices(case)
    assert raw[6] == vi["bytes_per_product"]
    if pal:
        assert 0 < vi["packed_slices"] < _slices(case) and vi["max_codes_per_slot"] > 16, vi
        with _context(ps.CASES[case][0], 0) as c0:
            v0 = _product(c0, case, 0)
        assert v0["bytes_per_product"] - vi["bytes_per_product"] == 512 * vi["packed_slices"]


@pytest.mark.parametrize("pal", [1, 0])
def test_sixteen_and_seventeen_values_in_one_slot(pal):
    """exactly 16 distinct values in one slot of one slice: packed, like every other slice.  17: that slice alone is not, its
    neighbours are, its pair is a mixed one."""
    n = _slices("sixteen")
    with _context("p1_17", pal) as c:
        a = _product(c, "sixteen", pal)
        b = _product(c, "seventeen", pal)
    if pal:
        assert (a["packed_slices"], a["unpacked_slices"], a["mixed_pairs"], a["max_codes_per_slot"]) == (n, 0, 0, 16), a
        assert (b["packed_slices"], b["unpacked_slices"], b["mixed_pairs"], b["max_codes_per_slot"]) == (n - 1, 1, 1, 17), b
        assert b["bytes_per_product"] - a["bytes_per_product"] >= 512


@pytest.mark.parametrize("pal", [1, 0])
def test_no_slice_packed(pal):
    """every slice with a slot of 40 or 64 distinct values (512 in all: the dictionary stays in LDS): the report says no slice is
    packed, the kernel reads 16-bit codes everywhere, the bits are the serial loop's"""
    with _context("p1_10_9_11", pal) as c:
        vi = _product(c, "none_packed", pal)
    assert (vi["packed_slices"], vi["unpacked_slices"], vi["mixed_pairs"]) == (0, _slices("none_packed"), 0), vi
    if pal:
        assert vi["max_codes_per_slot"] == 64, vi


@pytest.mark.parametrize("pal", [1, 0])
def test_hostile_bits_in_the_palettes(pal):
    """a subnormal, +-inf, NaN, DBL_MAX, DBL_MIN in the palettes of two packed slices of a pair (-0.0 is an exact zero to the
    packer and leaves a hole): NaN exactly where the serial loop has it"""
    with _context("p1_17", pal) as c:
        vi = _product(c, "hostile", pal)
    if pal:
        assert (vi["packed_slices"], vi["unpacked_slices"]) == (_slices("hostile"), 0), vi
    assert np.isnan(_reference("hostile")[1]).any()


def test_one_context_across_uploads():
    """packed values, then the 17-value case, then the first again, then values no slice can pack, then the first: palettes,
    marks and byte counts follow every upload"""
    n = _slices("sixteen")
    with _context("p1_17", 1) as c:
        seen = [_product(c, case, 1) for case in ("sixteen", "seventeen", "sixteen", "assembled_p1_17", "tame")]
    assert [v["unpacked_slices"] for v in seen[:3]] == [0, 1, 0] and [v["mixed_pairs"] for v in seen[:3]] == [0, 1, 0]
    assert seen[0]["bytes_per_product"] == seen[2]["bytes_per_product"] < seen[1]["bytes_per_product"]
    assert 0 < seen[3]["unpacked_slices"] < n and (seen[4]["packed_slices"], seen[4]["max_codes_per_slot"]) == (n, 5)


@pytest.mark.parametrize("case", ["seventeen", "hostile", "none_packed"])
def test_dot_forms_with_the_knob_on_and_off(case):
    """the kernels that also sum <p, A p> (classical) and the single reduction's three sums, eight iterations on the case's values
    (a mixed pair; NaN and inf; nothing packed): whatever the iteration makes of them, knob 1 and knob 0 make the same bits"""
    res = {}
    for pal in (1, 0):
        with _context(ps.CASES[case][0], pal) as c:
            c.csr_upload_values(ps.values(case))
            res[pal] = []
            for sr in (False, True):
                it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-30, max_it=8, single_reduction=sr)
                res[pal].append((it, c.cg_reason(), c.cg_history(it + 1), c.vec_download(zzz.VEC_U)))
    for p, q in zip(res[1], res[0]):
        assert p[:2] == q[:2]
        np.testing.assert_array_equal(p[2].view(np.uint64), q[2].view(np.uint64))
        np.testing.assert_array_equal(p[3].view(np.uint64), q[3].view(np.uint64))


def _solve_all(c):
    out = []
    for sr in (False, True):
        it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, single_reduction=sr)
        assert c.cg_reason() == 2 and rn <= 1e-8 * r0
        out.append(dict(it=it, rn=rn, r0=r0, u=c.vec_download(zzz.VEC_U), hist=c.cg_history(it + 1)))
    return out


@pytest.mark.parametrize("name", ["p1_17", "p1_10_9_11"])
def test_solves_with_the_knob_on_and_off(name):
    """Jacobi-CG, classical and single reduction, on the assembled matrix (packed, unpacked and mixed pairs in one stream): knob 1
    against 0 identical in iterations, residual history and every bit of u; both within the project's bars of the oracle's"""
    _, rp, cl, _ = ps.problem(name)
    res = {}
    for pal in (1, 0):
        with _context(name, pal) as c:
            vi = c.spmv_values_info()
            assert vi["one_chunk_kernel"] and (vi["packed_slices"] > 0) == (pal == 1), vi
            res[pal] = _solve_all(c)
            _, _, v = c.csr_download()
            b = c.vec_download(zzz.VEC_B)
    for p, q in zip(res[1], res[0]):
        assert (p["it"], p["rn"], p["r0"]) == (q["it"], q["rn"], q["r0"])
        np.testing.assert_array_equal(p["hist"].view(np.uint64), q["hist"].view(np.uint64))
        np.testing.assert_array_equal(p["u"].view(np.uint64), q["u"].view(np.uint64))
    oit, ou, _, _ = zo.pcg(rp, cl, v, b, rtol=1e-8)
    sit, su, _, _ = zo.pcg_single_reduction(rp, cl, v, b, rtol=1e-8)
    for r in (res[1], res[0]):
        assert abs(r[0]["it"] - oit) <= 2 and np.linalg.norm(r[0]["u"] - ou) <= 1e-6 * np.linalg.norm(ou)
        assert abs(r[1]["it"] - sit) <= 2 and np.linalg.norm(r[1]["u"] - su) <= 1e-6 * np.linalg.norm(su)


def test_two_way_partition_with_the_knob_on_and_off():
    """two z-slabs of the small lattice, both ranks on this GPU through the host-mediated communicator: the interior and boundary
    slice lists of the overlapped product reach packed and unpacked slices; knob 1 against 0, every rank, the same bits"""
    import threading

    nparts, dims = 2, ps.PROBLEMS["p1_10_9_11"][2]

    def partitioned(pal):
        grp = zzz.LocalGroup(nparts)
        out, err = [None] * nparts, []

        def run(rank):
            try:
                P = zzz.Part("poisson", 1, *dims, nparts, rank)
                with zzz.Context(0) as c:
                    c.comm_init_local(grp.h, rank)
                    c.upload_part(P)
                    c.upload_halo(P)
                    c.pattern_build()
                    c.assemble_matrix(P.form)
                    c.assemble_vector(P.form)
                    res = []
                    for sr in (False, True):
                        it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, single_reduction=sr)
                        res.append((it, rn, r0, c.cg_history(it + 1), c.vec_download(zzz.VEC_U)))
                    out[rank] = (res, c.spmv_values_info())
            except Exception as e:  # noqa: BLE001
                err.append((rank, repr(e)))

        with _Env(**FORCED):
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("ZZZ_SELLP_PAL", str(pal))
                th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
                for t in th:
                    t.start()
                for t in th:
                    t.join(timeout=300)
        grp.close()
        assert not err, err
        assert all(o is not None for o in out)
        return out

    new, ref = partitioned(1), partitioned(0)
    for rank in range(nparts):
        assert new[rank][1]["one_chunk_kernel"] and new[rank][1]["packed_slices"] > 0 and ref[rank][1]["packed_slices"] == 0, new[rank][1]
        for p, q in zip(new[rank][0], ref[rank][0]):
            assert p[:3] == q[:3]
            np.testing.assert_array_equal(p[3].view(np.uint64), q[3].view(np.uint64))
            np.testing.assert_array_equal(p[4].view(np.uint64), q[4].view(np.uint64))
