"""Build-time guard for the vector kernel of the pipelined CG (csrc/zzz_cg_pipe.hip), in the manner of
tests/test_kernel_resources.py: k_pipe_update keeps eight 16-B streams in flight per lane ahead of its scalar prologue, which
costs registers -- it must stay within the 128 VGPRs of four wavefronts per SIMD (what its measured 6.8 TB/s at C2 ran with),
without scratch, and four of its workgroups (with the table of the coded inverse diagonal) must fit a CU's 160 KB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pipecg_update_kernel_resources(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_cg_pipe.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if not re.match(r"_ZN3zzz13k_pipe_updateILb[01]ELb[01]EEE", name):
            continue
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert vgprs <= 128 and occ >= 4 and scratch == 0, (name, vgprs, occ, scratch)
        assert lds * 4 <= 160 * 1024, (name, lds)
        seen += 1
    assert seen == 4  # load policy x (inverse diagonal as doubles | as codes)
