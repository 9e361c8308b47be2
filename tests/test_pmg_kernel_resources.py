"""Build-time guard for the transfer kernels of the p-multigrid preconditioner (csrc/zzz_pmg.hip), in the manner of
tests/test_mg_kernel_resources.py: a thread selects up to 65 entity indices per component from zzzcube::Layout -- written so
that the masks are constants and the selection stays in registers -- so none of the kernels may touch scratch memory, and
both, which gather, must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, ROOT, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pmg_kernels_have_no_scratch_and_keep_four_waves():
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_pmg.hip")
    assert os.path.exists(src), "csrc/zzz_pmg.hip: the transfer kernels of ZZZ_PC_PMG are not there"
    seen = set()
    for name, k in kernel_resources("zzz_pmg.hip").items():
        # _ZN3zzz13k_pmg_prolongILi2ELi1EEEv...: the kernel and its <ORDER, BS>
        m = re.match(r"_ZN3zzz\d+(k_pmg_[a-z]+)ILi(\d)ELi(\d)EEE", name)
        if not m:
            assert "k_pmg_" not in name, name
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen.add((m.group(1), int(m.group(2)), int(m.group(3))))
    # prolongation and restriction, each for order 2 and 3 and block size 1 and 3
    assert seen == {(k, o, bs) for k in ("k_pmg_prolong", "k_pmg_restrict") for o in (2, 3) for bs in (1, 3)}
