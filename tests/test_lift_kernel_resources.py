"""Build-time guard for the lifting pass (csrc/zzz_assemble.hip: k_lift), in the manner of
tests/test_mg_kernel_resources.py: a lane holds its columns' dofs, Dirichlet bits, values of u0, the cell's geometry and
up to nine element entries per column -- all in registers, selected by compile-time indices -- so no instantiation may
touch scratch memory or spill, and each, which chases adjacency -> connectivity -> flags and values, must keep at least four
wavefronts per SIMD (registers and the reference tensors in LDS both counted) to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lift_kernels_have_no_scratch_and_keep_four_waves():
    seen = set()
    for name, k in kernel_resources("zzz_assemble.hip").items():
        # _ZN3zzz6k_liftILi20ELi3ELi8EEEv...: the kernel and its <ND, BS, LPR>
        m = re.match(r"_ZN3zzz\d+k_liftILi(\d+)ELi(\d)ELi(\d)EEE", name)
        if not m:
            assert "k_liftI" not in name, name
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen.add(tuple(int(v) for v in m.groups()))
    # P1, P2, P3 (4, 10, 20 dofs per cell), Poisson and elasticity, with the lanes per row launch_lift picks
    assert seen == {(4, 1, 1), (4, 3, 1), (10, 1, 2), (10, 3, 4), (20, 1, 4), (20, 3, 8)}
