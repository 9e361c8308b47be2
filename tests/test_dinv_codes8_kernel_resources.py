"""Build-time guard for the vector kernels that read Jacobi's inverse diagonal as 8-bit codes (the `_c8` entry points of
csrc/zzz_cg.hip and csrc/zzz_cg_pipe.hip), in the manner of tests/test_cg_vector_kernel_resources.py.  It reads resource
figures only.  The kernels are bound by HBM bytes, so what matters is that none of them touches scratch memory and that none
runs at a lower occupancy, or with a larger LDS table, than the 16-bit form of the same kernel in the same compile (the
table shrinks from 2 048 to 256 entries)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# the 8-bit entry point -> (source file, the 16-bit instantiation with the same load policy NT, as mangled template arguments)
_PAIRS = {
    "k_update_xr_c8": ("zzz_cg.hip", "k_update_xr", "Lb{nt}ELb1E"),
    "k_update_p_c8": ("zzz_cg.hip", "k_update_p", "Lb{nt}ELb1E"),
    "k_update_p_light_c8": ("zzz_cg.hip", "k_update_p_light", "Lb{nt}ELb1E"),
    "k_update_p_flush_c8": ("zzz_cg.hip", "k_update_p_flush", "Lb{nt}ELb1ELi{k}E"),
    "k_sr_update_c8": ("zzz_cg.hip", "k_sr_update", "Lb{nt}ELb0ELb1E"),
    "k_pipe_update_c8": ("zzz_cg_pipe.hip", "k_pipe_update", "Lb{nt}ELb1E"),
}


def _resources(src_name, tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", src_name)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / (src_name + ".o")),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        m = re.match(r"_ZN3zzz\d+(k_[a-z0-9_]+)I((?:L[bi]\d+E)+)EE", b.split()[0])
        if not m:
            continue
        found[(m.group(1), m.group(2))] = dict(
            occ=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)),
            scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)),
            vspill=int(re.search(r"VGPRs Spill: (\d+)", b).group(1)),
            sspill=int(re.search(r"SGPRs Spill: (\d+)", b).group(1)),
            lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)),
            vgprs=int(re.search(r"VGPRs: (\d+)", b).group(1)))
    return found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src_name", ["zzz_cg.hip", "zzz_cg_pipe.hip"])
def test_8bit_code_kernels_have_no_scratch_and_keep_the_16bit_occupancy(src_name, tmp_path):
    found = _resources(src_name, tmp_path)
    seen = 0
    for kern, (src, wide, wide_args) in _PAIRS.items():
        if src != src_name:
            continue
        for nt in (0, 1):
            for k in ((2, 4, 8) if "flush" in kern else (None,)):
                args8 = f"Lb{nt}E" + (f"Li{k}E" if k else "")
                assert (kern, args8) in found, (kern, args8, sorted(x for x in found if x[0] == kern))
                a, b = found[(kern, args8)], found[(wide, wide_args.format(nt=nt, k=k))]
                print(kern, args8, a, "| 16-bit:", b)
                assert a["scratch"] == 0 and a["vspill"] == 0 and a["sspill"] == 0, (kern, args8, a)
                assert a["occ"] >= b["occ"], (kern, args8, a, b)
                # 2 048 - 256 table entries of 8 B fewer
                assert a["lds"] == b["lds"] - (2048 - 256) * 8, (kern, args8, a["lds"], b["lds"])
                seen += 1
    assert seen == (2 * (3 + 3 + 1) if src_name == "zzz_cg.hip" else 2)
