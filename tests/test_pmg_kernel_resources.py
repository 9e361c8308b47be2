"""Build-time guard for the transfer kernels of the p-multigrid preconditioner (csrc/zzz_pmg.hip), in the manner of
tests/test_mg_kernel_resources.py: a thread selects up to 65 entity indices per component from zzzcube::Layout -- written so
that the masks are constants and the selection stays in registers -- so none of the kernels may touch scratch memory, and
both, which gather, must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pmg_kernels_have_no_scratch_and_keep_four_waves(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_pmg.hip")
    assert os.path.exists(src), "csrc/zzz_pmg.hip: the transfer kernels of ZZZ_PC_PMG are not there"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fopenmp", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        # _ZN3zzz13k_pmg_prolongILi2ELi1EEEv...: the kernel and its <ORDER, BS>
        m = re.match(r"_ZN3zzz\d+(k_pmg_[a-z]+)ILi(\d)ELi(\d)EEE", name)
        if not m:
            assert "k_pmg_" not in name, name
            continue
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sspill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        print(name, "VGPRs", vgprs, "occupancy", occ, "scratch", scratch, "spills", vspill, sspill)
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert occ >= 4 and vgprs <= 128, (name, vgprs, occ)
        seen.add((m.group(1), int(m.group(2)), int(m.group(3))))
    # prolongation and restriction, each for order 2 and 3 and block size 1 and 3
    assert seen == {(k, o, bs) for k in ("k_pmg_prolong", "k_pmg_restrict") for o in (2, 3) for bs in (1, 3)}
