"""Build-time guard for the direction kernels of the classical CG loop (csrc/zzz_cg.hip), in the manner of
tests/test_kernel_resources.py: k_update_p in place and its two forms with the solution update deferred (k_update_p_light,
k_update_p_flush<.., K>), plus the pass that applies what is pending when a solve ends (k_x_apply_pending<K>).  They are
bound by HBM bytes, so what matters is that none of them touches scratch memory, and that neither deferred form runs at
a lower occupancy than the in-place kernel the headline ran with until now, k_update_p<true, true>, in the same compile
(the flush form holds K alphas and reads K - 1 more vectors per entry)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_direction_kernels_have_no_scratch_and_keep_the_in_place_occupancy(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_cg.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    found = {}
    for b in blocks:
        name = b.split()[0]
        m = re.match(r"_ZN3zzz\d+(k_update_p|k_update_p_light|k_update_p_flush|k_x_apply_pending)I((?:L[bi]\d+E)+)EE", name)
        if not m:
            continue
        args = tuple(int(a) for a in re.findall(r"L[bi](\d+)E", m.group(2)))
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        sspill = int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
        print(m.group(1), args, "VGPRs", vgprs, "occupancy", occ, "scratch", scratch, "spills", vspill, sspill)
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        found[(m.group(1), args)] = occ
    flags = [(nt, dz) for nt in (0, 1) for dz in (0, 1)]
    # every instantiation the solver can launch is there: load policy x (inverse diagonal as doubles | as codes) [x K]
    assert {k for k in found if k[0] == "k_update_p"} == {("k_update_p", f) for f in flags}
    assert {k for k in found if k[0] == "k_update_p_light"} == {("k_update_p_light", f) for f in flags}
    assert {k for k in found if k[0] == "k_update_p_flush"} == {("k_update_p_flush", f + (K,)) for f in flags for K in (2, 4, 8)}
    assert {k for k in found if k[0] == "k_x_apply_pending"} == {("k_x_apply_pending", (K,)) for K in (2, 4, 8)}
    base = found[("k_update_p", (1, 1))]
    for (kern, args), occ in found.items():
        if kern in ("k_update_p_light", "k_update_p_flush"):
            assert occ >= base, (kern, args, occ, base)
