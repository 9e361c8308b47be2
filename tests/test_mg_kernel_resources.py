"""Build-time guard for the kernels of the multigrid preconditioner (csrc/zzz_mg.hip), in the manner of
tests/test_kernel_resources.py: the transfer sorts three (fraction, axis) pairs per fine vertex -- written so that they stay
in registers -- and the restriction walks up to 64 fine vertices per lane; none of the kernels may touch scratch memory, and the
transfer kernels, which gather, must keep at least four wavefronts per SIMD to hide that latency."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mg_kernels_have_no_scratch_and_the_transfer_keeps_four_waves(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_mg.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fopenmp", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        m = re.match(r"_ZN3zzz\d+(k_mg_[a-z]+)", name)
        if not m:
            continue
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sspill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        print(name, "VGPRs", vgprs, "occupancy", occ, "scratch", scratch, "spills", vspill, sspill)
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        if m.group(1) in ("k_mg_prolong", "k_mg_restrict"):
            assert occ >= 4 and vgprs <= 128, (name, vgprs, occ)
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    # prolongation, restriction for block size 1 and 3, the smoother's two terms, the dense coarsest solve
    assert seen == {"k_mg_prolong": 1, "k_mg_restrict": 2, "k_mg_first": 1, "k_mg_term": 1, "k_mg_dense": 1}
