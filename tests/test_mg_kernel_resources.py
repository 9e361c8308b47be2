"""Build-time guard for the kernels of the multigrid preconditioner (csrc/zzz_mg.hip), in the manner of
tests/test_kernel_resources.py: the transfer sorts three (fraction, axis) pairs per fine vertex -- written so that they stay
in registers -- and the restriction walks up to 64 fine vertices per lane; none of the kernels may touch scratch memory, and the
transfer kernels, which gather, must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mg_kernels_have_no_scratch_and_the_transfer_keeps_four_waves():
    seen = {}
    # (the smoother's two kernels are the Chebyshev-Jacobi polynomial's, csrc/zzz_cg.hip)
    for name, k in list(kernel_resources("zzz_mg.hip").items()) + list(kernel_resources("zzz_cg.hip").items()):
        m = re.match(r"_ZN3zzz\d+(k_mg_[a-z]+|k_cheb_first|k_cheb_step)", name)
        if not m:
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        if m.group(1) in ("k_mg_prolong", "k_mg_restrict"):
            assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # prolongation, restriction for block size 1 and 3, the smoother's two terms, the dense coarsest solve
    assert seen == {"k_mg_prolong": 1, "k_mg_restrict": 2, "k_cheb_first": 1, "k_cheb_step": 1, "k_mg_dense": 1}
