"""Build-time guard for the transfer kernels of csrc/zzz_mg.hip since they walk a window of fine vertex planes (the whole cube,
or the z-slab a rank owns: csrc/zzz_mg_transfer.h): the window's four plane numbers travel in the kernel arguments and its clamp
is two compares per coarse vertex, so the kernels still use no scratch and no LDS and keep what
tests/test_mg_kernel_resources.py demands of them -- at least four wavefronts per SIMD, at most 128 vector registers -- and the
slab path adds no kernel of its own (prolongation once, restriction per block size)."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_windowed_transfer_kernels_keep_their_resources():
    seen = {}
    for name, k in kernel_resources("zzz_mg.hip").items():
        m = re.match(r"_ZN3zzz\d+(k_mg_prolong|k_mg_restrict)", name)
        if not m:
            continue
        print(name, k)
        assert "MgGeom" in name  # (the window is part of the level pair's geometry, passed by value)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 and k["lds"] == 0, (name, k)
        assert k["occ"] >= 4 and k["vgprs"] <= 128, (name, k)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    assert seen == {"k_mg_prolong": 1, "k_mg_restrict": 2}
