"""Build-time guard for the vector kernel of the pipelined CG (csrc/zzz_cg_pipe.hip), in the manner of
tests/test_kernel_resources.py: k_pipe_update keeps eight 16-B streams in flight per lane ahead of its scalar prologue, which
costs registers -- it must stay within the 128 VGPRs of four wavefronts per SIMD (what its measured 6.8 TB/s at C2 ran with),
without scratch, and four of its workgroups (with the table of the coded inverse diagonal) must fit a CU's 160 KB of LDS."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pipecg_update_kernel_resources():
    seen = 0
    for name, k in kernel_resources("zzz_cg_pipe.hip").items():
        # k_pipe_update<NT, DZ>, DZ = 0 and 1 (the 8-bit codes' smaller table: tests/test_dinv_codes8_kernel_resources.py)
        if not re.match(r"_ZN3zzz13k_pipe_updateILb[01]ELi[01]EEE", name):
            continue
        assert k["vgprs"] <= 128 and k["occ"] >= 4 and k["scratch"] == 0, (name, k)
        assert k["lds"] * 4 <= 160 * 1024, (name, k)
        seen += 1
    assert seen == 4  # load policy x (inverse diagonal as doubles | as 16-bit codes)
