"""Build-time guard for the kernels of the aggregation multigrid (csrc/zzz_agg.hip), in the manner of
tests/test_mg_kernel_resources.py: the rounds of the independent set, the joins and the transfers are one thread per node over
CSR rows with loads at clamped indices and selects -- no indexed private array, so none of them may touch scratch memory; none
uses LDS; and the kernels that gather (the rounds, the joins, the Galerkin sum, the two transfers) must keep at least four
wavefronts per SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources

GATHER = ("k_agg_max1", "k_agg_max2", "k_agg_near1", "k_agg_near2", "k_agg_join", "k_agg_values", "k_agg_restrict", "k_agg_prolong")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_agg_kernels_have_no_scratch_no_lds_and_the_gathers_keep_four_waves():
    seen = {}
    for name, k in kernel_resources("zzz_agg.hip").items():
        m = re.match(r"_ZN3zzz\d+(k_agg_[a-z0-9_]+?)(?:I|E)", name)
        if not m:
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 and k["lds"] == 0, (name, k)
        if m.group(1) in GATHER:
            assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # block size 1 and 3 of everything that walks block rows, the two sort-key kernels and the transfers; one of the rest;
    # the offsets for the members (32-bit) and for the coarse row pointers (64-bit)
    assert seen == {"k_agg_init": 2, "k_agg_max1": 2, "k_agg_max2": 2, "k_agg_near1": 2, "k_agg_near2": 2, "k_agg_join": 2,
                    "k_agg_caller_keys": 2, "k_agg_coarse_keys": 2, "k_agg_restrict": 2, "k_agg_prolong": 2, "k_agg_flags": 1,
                    "k_agg_number": 1, "k_agg_member_keys": 1, "k_agg_offsets": 2, "k_agg_rowidx": 1, "k_agg_heads": 1,
                    "k_agg_entries": 1, "k_agg_values": 1, "k_agg_rowstats": 1}
