"""Build-time guard for the kernels of the smoothed-aggregation multigrid (csrc/zzz_sagg.hip), in the manner of
tests/test_agg_kernel_resources.py: every kernel is one thread per row, entry or run with loads at computed indices and no indexed
private array, so none may touch scratch memory; none uses LDS; and the kernels that gather through an index (the sums behind P,
A P and P^T (A P), and the two transfers of the cycle) must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources

GATHER = ("k_sagg_p_values", "k_sagg_sum_products", "k_sagg_gather", "k_sagg_restrict", "k_sagg_prolong")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sagg_kernels_have_no_scratch_no_lds_and_the_gathers_keep_four_waves():
    seen = {}
    for name, k in kernel_resources("zzz_sagg.hip").items():
        m = re.match(r"_ZN3zzz\d+(k_sagg_[a-z0-9_]+?)(?:I|E)", name)
        if not m:
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 and k["lds"] == 0, (name, k)
        if m.group(1) in GATHER:
            assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # block size 1 and 3 of what turns a dof into its coarse dof or into the caller's numbering; one of the rest
    assert seen == {"k_sagg_rowidx": 1, "k_sagg_caller_keys": 2, "k_sagg_p_keys": 2, "k_sagg_heads": 1, "k_sagg_entries": 1,
                    "k_sagg_offsets": 1, "k_sagg_r_keys": 2, "k_sagg_r_entries": 1, "k_sagg_t_count": 1, "k_sagg_t_terms": 2,
                    "k_sagg_t_rows": 1, "k_sagg_c_count": 1, "k_sagg_c_terms": 1, "k_sagg_diag": 1, "k_sagg_p_values": 2,
                    "k_sagg_gather": 1, "k_sagg_sum_products": 1, "k_sagg_rowstats": 1, "k_sagg_restrict": 1, "k_sagg_prolong": 1}
