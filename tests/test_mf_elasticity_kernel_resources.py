"""Build-time guard for the block-size-3 instantiations of the matrix-free action (k_mf_action3<ND, T, DIAG> of
csrc/zzz_matfree.hip), in the manner of tests/test_f32_kernel_resources.py: the file is compiled for gfx950 and the compiler's
resource report is read.

  * P1 (ND = 4) and P2 (ND = 10), action and diagonal, every workgroup size offered (128, 256, 512): no scratch, no spill.
  * P3 (ND = 20): the element holds g for all modes (90 doubles) beside u_e of one component, then y_e of the three; the
    build gives, for T = 128 / 256 / 512 alike,

        action    256 VGPRs, 0 AGPRs, 2 waves per SIMD, 2188 B of scratch per lane, 679 spilled VGPRs, 9632 .. 9664 B static LDS
        diagonal  256 VGPRs, 0 AGPRs, 2 waves per SIMD, no scratch,                                  4832 .. 4864 B static LDS

    asserted here as upper bounds: a regression guard, not an acceptance number (DESIGN.md 4f says what was tried).
  * No instantiation for 1024 threads exists at block size 3 (128 registers per lane do not hold a P2 element).
"""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_block_size_3_action_resources():
    res = kernel_resources("zzz_matfree.hip")
    seen = {}
    for name, k in res.items():
        m = re.search(r"k_mf_action3ILi(\d+)ELi(\d+)ELb([01])E", name)
        if not m:
            continue
        nd, t, diag = int(m.group(1)), int(m.group(2)), int(m.group(3))
        print(nd, t, diag, k)
        seen[(nd, t, diag)] = k
    assert sorted(seen) == sorted((nd, t, d) for nd in (4, 10, 20) for t in (128, 256, 512) for d in (0, 1))
    for (nd, t, diag), k in seen.items():
        assert k["sspill"] == 0, (nd, t, diag, k)
        if nd != 20 or diag:
            assert k["scratch"] == 0 and k["vspill"] == 0, (nd, t, diag, k)
        if nd == 20:
            assert k["vgprs"] + k["agprs"] <= 256 and k["occ"] >= 2, (t, diag, k)
            assert k["lds"] <= (4864 if diag else 9664), (t, diag, k)
            if not diag:
                assert k["scratch"] <= 2188 and k["vspill"] <= 679, (t, k)
    fin = [k for n, k in res.items() if "k_mf_finish3" in n or "k_mf_geom_el" in n]
    assert len(fin) == 2 and all(k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 for k in fin)
