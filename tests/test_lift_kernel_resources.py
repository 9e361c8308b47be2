"""Build-time guard for the lifting pass (csrc/zzz_assemble.hip: k_lift), in the manner of
tests/test_mg_kernel_resources.py: a lane holds its columns' dofs, Dirichlet bits, values of u0, the cell's geometry and
up to nine element entries per column -- all in registers, selected by compile-time indices -- so no instantiation may
touch scratch memory or spill, and each, which chases adjacency -> connectivity -> flags and values, must keep at least four
wavefronts per SIMD (registers and the reference tensors in LDS both counted) to hide that latency."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lift_kernels_have_no_scratch_and_keep_four_waves(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_assemble.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fopenmp", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        # _ZN3zzz6k_liftILi20ELi3ELi8EEEv...: the kernel and its <ND, BS, LPR>
        m = re.match(r"_ZN3zzz\d+k_liftILi(\d+)ELi(\d)ELi(\d)EEE", name)
        if not m:
            assert "k_liftI" not in name, name
            continue
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sspill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(name, "VGPRs", vgprs, "occupancy", occ, "scratch", scratch, "spills", vspill, sspill, "LDS", lds)
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert occ >= 4 and vgprs <= 128, (name, vgprs, occ)
        seen.add(tuple(int(v) for v in m.groups()))
    # P1, P2, P3 (4, 10, 20 dofs per cell), Poisson and elasticity, with the lanes per row launch_lift picks
    assert seen == {(4, 1, 1), (4, 3, 1), (10, 1, 2), (10, 3, 4), (20, 1, 4), (20, 3, 8)}
