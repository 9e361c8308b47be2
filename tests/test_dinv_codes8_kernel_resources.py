"""Build-time guard for the vector kernels that read Jacobi's inverse diagonal as 8-bit codes (the DZ = 2 instantiations of
csrc/zzz_cg.hip and csrc/zzz_cg_pipe.hip), in the manner of tests/test_cg_vector_kernel_resources.py.  It reads resource
figures only.  The kernels are bound by HBM bytes, so what matters is that none of them touches scratch memory and that none
runs at a lower occupancy, or with a larger LDS table, than the 16-bit form (DZ = 1) of the same kernel in the same compile
(the table shrinks from 2 048 to 256 entries)."""
import os

import pytest

from _kernel_resources import HIPCC, kernel_resources, template_args

# kernel -> (source file, its template arguments from the load policy NT, the diagonal's form DZ and the ring length K)
_KERNELS = {
    "k_update_xr": ("zzz_cg.hip", lambda nt, dz, k: (nt, dz)),
    "k_update_p": ("zzz_cg.hip", lambda nt, dz, k: (nt, dz)),
    "k_update_p_light": ("zzz_cg.hip", lambda nt, dz, k: (nt, dz)),
    "k_update_p_flush": ("zzz_cg.hip", lambda nt, dz, k: (nt, dz, k)),
    "k_sr_update": ("zzz_cg.hip", lambda nt, dz, k: (nt, 0, dz)),
    "k_pipe_update": ("zzz_cg_pipe.hip", lambda nt, dz, k: (nt, dz)),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src_name", ["zzz_cg.hip", "zzz_cg_pipe.hip"])
def test_8bit_code_kernels_have_no_scratch_and_keep_the_16bit_occupancy(src_name):
    found = {template_args(name): k for name, k in kernel_resources(src_name).items() if template_args(name)}
    seen = 0
    for kern, (src, args) in _KERNELS.items():
        if src != src_name:
            continue
        for nt in (0, 1):
            for k in ((2, 4, 8) if "flush" in kern else (None,)):
                assert (kern, args(nt, 2, k)) in found, (kern, args(nt, 2, k), sorted(x for x in found if x[0] == kern))
                a, b = found[(kern, args(nt, 2, k))], found[(kern, args(nt, 1, k))]
                print(kern, args(nt, 2, k), a, "| 16-bit:", b)
                assert a["scratch"] == 0 and a["vspill"] == 0 and a["sspill"] == 0, (kern, nt, k, a)
                assert a["occ"] >= b["occ"], (kern, nt, k, a, b)
                # 2 048 - 256 table entries of 8 B fewer
                assert a["lds"] == b["lds"] - (2048 - 256) * 8, (kern, nt, k, a["lds"], b["lds"])
                seen += 1
    assert seen == (2 * (3 + 3 + 1) if src_name == "zzz_cg.hip" else 2)
