"""Build-time guard for the kernels of the smoothed aggregation with rigid-body modes (csrc/zzz_sagg_rbm.hip), in the manner of
tests/test_sagg_kernel_resources.py: the orthogonalisation is a wavefront per aggregate whose lanes loop over rows in memory
with its six columns unrolled and its kept-column set one register, the others are one thread per dof, entry or run with loads
at computed (always valid) indices and selects -- no indexed private array, so none may touch scratch memory; none uses LDS
(the orthogonalisation exchanges through the shuffle tree alone); and the kernels that gather through an index
must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources

GATHER = ("k_srbm_b0", "k_srbm_gather_rows", "k_srbm_qr", "k_srbm_p_count", "k_srbm_p_terms", "k_srbm_p_values", "k_srbm_drop_list",
          "k_srbm_member_pos")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sagg_rbm_kernels_have_no_scratch_no_lds_and_the_gathers_keep_four_waves():
    seen = {}
    for name, k in kernel_resources("zzz_sagg_rbm.hip").items():
        m = re.match(r"_ZN3zzz\d+(k_srbm_[a-z0-9_]+?)(?:I|E)", name)
        if not m:
            assert "k_sagg_" not in name and "k_agg_" not in name, f"{name}: the shared kernels stay in their own translation units"
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 and k["lds"] == 0, (name, k)
        if m.group(1) in GATHER:
            assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # node size 3 and 6 of what turns a dof into its node; one of the rest
    assert seen == {"k_srbm_b0": 1, "k_srbm_member_pos": 1, "k_srbm_gather_rows": 2, "k_srbm_qr": 1, "k_srbm_drop_list": 1,
                    "k_srbm_p_count": 2, "k_srbm_p_terms": 2, "k_srbm_p_values": 2, "k_srbm_node_rows": 1, "k_srbm_node_cols": 1,
                    "k_srbm_unit_terms": 1}
