"""Build-time guard: the CG SpMV kernel owes ~20 % of its speed to running 8 wavefronts per SIMD
(measured: a change that raised it from 64 to 78 VGPRs took the 10 M-dof SpMV from 0.396 to 0.486 ms), and
it sits exactly at the 64-VGPR limit of that occupancy.  hipcc cross-compiles without a GPU, so the register
count of the shipped variants is checked here, where a regression is cheap to see."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_spmv_tile_kernel_keeps_full_occupancy():
    seen = 0
    for name, k in kernel_resources("zzz_spmv.hip").items():
        # spmv_tile_kernel<DOT, NT>: the four variants the solver launches
        if not re.match(r"_ZN3zzz16spmv_tile_kernelILb([01])ELb([01])EEE", name):
            continue
        assert k["vgprs"] <= 64 and k["occ"] == 8 and k["vspill"] == 0, (name, k)
        assert k["lds"] * 8 <= 160 * 1024, (name, k)  # eight workgroups per CU must fit the 160 KB of LDS
        seen += 1
    assert seen == 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_operator_stream_kernel_keeps_full_occupancy():
    """The product on the operator stream (zzz_sellp.hip) has no LDS and must stay at 8 wavefronts per SIMD (<= 64 VGPRs:
    its launch bound); without spills it would need 74 registers = 6 wavefronts, measured exactly as fast, so the few
    spilled dwords are tolerated -- but not growth beyond that."""
    seen = 0
    for name, k in kernel_resources("zzz_sellp.hip").items():
        if not re.match(r"_ZN3zzz17spmv_sellp_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb[01]ELi[0123]EEE", name):
            continue
        # LDS: the cross-wavefront sums, a few hundred bytes per workgroup;
        # SGPRs <= 80 keeps eight 256-thread workgroups per CU admissible (MI355X_MICROARCH.md, Residency)
        assert k["vgprs"] <= 64 and k["occ"] == 8 and k["scratch"] <= 64 and k["lds"] <= 512 and k["sgprs"] <= 80, (name, k)
        seen += 1
    # (dot products, load policy, row permutation, Chebyshev-term epilogue) + x windows (natural order), each with the
    # values as doubles, as codes into a dictionary in memory, as codes into a dictionary in LDS, as 8-bit codes into
    # per-slice dictionaries
    assert seen == 88  # (slice dictionaries and x windows exclude each other)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src_name,kernel_re,lds_budget,variants", [
    ("zzz_sellp_blk.hip", r"_ZN3zzz16spmv_blk3_kernelILb[01]ELb[01]ELb[01]ELi[12]ELb[01]EEE", 2200 * 72, 20),
    ("zzz_sellp_win.hip", r"_ZN3zzz15spmv_win_kernelILb[01]ELb[01]ELb[01]ELb[01]EEE", (11264 + 8192) * 8, 10)])
def test_special_product_kernels_fit_one_workgroup_of_1024_lanes_per_cu(src_name, kernel_re, lds_budget, variants):
    """The block-row and block-window products (round 6) run ONE workgroup of 1 024 lanes per CU: sixteen wavefronts, four per SIMD,
    i.e. at most 128 VGPRs per lane, with (nearly) no scratch; their dynamic LDS (block table / window + dictionary) plus the static
    part must fit the CU's 160 KB."""
    seen = 0
    for name, k in kernel_resources(src_name).items():
        if not re.match(kernel_re, name):
            continue
        assert k["vgprs"] <= 128 and k["occ"] >= 4 and k["scratch"] <= 64, (name, k)
        assert k["lds"] + lds_budget <= 160 * 1024, (name, k)
        seen += 1
    assert seen == variants, seen  # (dot / single reduction / load policy [/ table form], and the Chebyshev-epilogue variants)
