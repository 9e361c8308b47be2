"""Build-time guard for the single-precision cgpoisson path, in the manner of tests/test_mg_kernel_resources.py: the float
instantiations of the matrix-free action (csrc/zzz_matfree.hip) and the float CG's vector kernels (csrc/zzz_cg_f32.hip) are
compiled for gfx950.  No float instantiation may touch scratch memory or spill a register; the float P3 action -- half the
registers of the double one for u_e, y_e and the table entries in flight -- must keep at least the double P3 action's
wavefronts per SIMD in the same compile; the three vector kernels of the float CG stay within the 64 registers of full
occupancy."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_float_action_has_no_scratch_and_p3_keeps_the_double_kernels_occupancy():
    res = kernel_resources("zzz_matfree.hip")
    seen, nfloat = {}, 0
    for name, k in res.items():
        # k_mf_action<ND, T, DIAG, R>: R is the last template argument, d or f
        m = re.search(r"k_mf_actionILi(\d+)ELi(\d+)ELb([01])E([df])E", name)
        if m:
            nd, t, diag, r = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
        elif re.search(r"k_mf_finishIfE|k_mf32_", name):
            nd, t, diag, r = 0, 0, 0, "f"
        else:
            continue
        print(name, k)
        if r == "f":
            nfloat += 1
            assert diag == 0, name  # the diagonal stays double
            assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        seen[(nd, t, diag, r)] = k
    for nd in (4, 10, 20):
        for t in (128, 256, 512, 1024):
            assert (nd, t, 0, "f") in seen and (nd, t, 0, "d") in seen, (nd, t)
    for t in (128, 256, 512, 1024):
        assert seen[(20, t, 0, "f")]["occ"] >= seen[(20, t, 0, "d")]["occ"], (t, seen[(20, t, 0, "f")], seen[(20, t, 0, "d")])
    assert nfloat == 12 + 4  # the action's, its finish, the three twin builders (rounding, P1 origins, P1 coordinates)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_float_cg_vector_kernels_keep_full_occupancy():
    res = kernel_resources("zzz_cg_f32.hip")
    seen = set()
    for name, k in res.items():
        m = re.search(r"\d+(k32_[a-z_]+?)E[iPK]", name)
        if not m:
            continue
        print(name, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["vgprs"] <= 64, (name, k)
        seen.add(m.group(1))
    assert {"k32_init", "k32_update_xr", "k32_update_p"} <= seen, seen
