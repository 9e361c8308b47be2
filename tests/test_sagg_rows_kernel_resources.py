"""Build-time guard for the kernels of the row-by-row products (csrc/zzz_sagg_rows.hip), in the manner of
tests/test_sagg_kernel_resources.py: the exact kernel set; none touches scratch memory or spills (the sources of P_t's rows
unroll their six columns into selects, the searches keep their bounds in registers); the numeric kernel's accumulators are the
one use of LDS -- the 32 KiB per workgroup of four wavefronts that its comment documents, five workgroups per CU -- and it,
the two value kernels of P and the candidate kernels, which all gather through an index, keep at least four wavefronts per
SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources

NUMERIC = ("k_srow_numeric", "k_srow_p_values_unit", "k_srow_p_values_rbm")
LDS = {"k_srow_numeric": 4 * 1024 * 8}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sagg_rows_kernels_have_no_scratch_and_the_numeric_ones_keep_four_waves():
    seen = {}
    for name, k in kernel_resources("zzz_sagg_rows.hip").items():
        m = re.match(r"_ZN3zzz\d+(k_srow_[a-z0-9_]+?)(?:I|E)", name)
        if not m:
            assert "k_sagg_" not in name and "k_srbm_" not in name and "k_agg_" not in name, \
                f"{name}: the shared kernels stay in their own translation units"
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["lds"] == LDS.get(m.group(1), 0), (name, k)
        if m.group(1) in NUMERIC or m.group(1) == "k_srow_candidates":
            assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # count and candidates: one per source of B's rows (a CSR, ZZZ_PC_SAGG's P_t, ZZZ_PC_SAGG_RBM's P_t); one of the rest
    assert seen == {"k_srow_ord_keys": 1, "k_srow_count": 3, "k_srow_candidates": 3, "k_srow_heads": 1, "k_srow_compact": 1,
                    "k_srow_rows": 1, "k_srow_p_values_unit": 1, "k_srow_p_values_rbm": 1, "k_srow_numeric": 1}
