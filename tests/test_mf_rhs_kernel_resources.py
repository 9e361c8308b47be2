"""Build-time guard for the cell-block right-hand side (k_mf_rhs<ND, T, BS> of csrc/zzz_matfree.hip), in the manner of
tests/test_mf_elasticity_kernel_resources.py: the file is compiled for gfx950 and the compiler's resource report is read.

  * Every instantiation the host dispatch names is there: ND in {4, 10, 20} x T in {128, 256, 512} at both block sizes, and
    T = 1024 at block size 1.
  * No SGPR spill anywhere; no scratch and no VGPR spill in any instantiation.
  * Occupancy (waves per SIMD) at least that of the action kernel of the same ND, T and block size in the same compile
    (k_mf_action<ND, T, false, double> at block size 1, k_mf_action3<ND, T, false> at block size 3).
  * The two lifting kernels: no scratch, no spill.
"""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_cell_block_rhs_resources():
    res = kernel_resources("zzz_matfree.hip")
    rhs, action, lift = {}, {}, []
    for name, k in res.items():
        m = re.search(r"k_mf_rhsILi(\d+)ELi(\d+)ELi([13])EE", name)
        if m:
            rhs[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = k
            continue
        m = re.search(r"k_mf_actionILi(\d+)ELi(\d+)ELb0EdE", name)
        if m:
            action[(int(m.group(1)), int(m.group(2)), 1)] = k
        m = re.search(r"k_mf_action3ILi(\d+)ELi(\d+)ELb0EE", name)
        if m:
            action[(int(m.group(1)), int(m.group(2)), 3)] = k
        if "k_mf_lift_" in name:
            lift.append(k)
    want = sorted([(nd, t, bs) for nd in (4, 10, 20) for t in (128, 256, 512) for bs in (1, 3)] + [(nd, 1024, 1) for nd in (4, 10, 20)])
    assert sorted(rhs) == want
    assert sorted(action) == want  # (what the occupancies below are compared with)
    bad = []
    for key in want:
        k, a = rhs[key], action[key]
        print(key, k, "| action occupancy", a["occ"])
        if k["sspill"] or k["scratch"] or k["vspill"] or k["occ"] < a["occ"]:
            bad.append((key, k, a["occ"]))
    assert not bad, bad
    assert len(lift) == 2 and all(k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0 for k in lift)
