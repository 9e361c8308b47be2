"""Build-time guard for the assembly kernels (csrc/zzz_assemble.hip with csrc/zzz_asm_elem.h), in the manner of
tests/test_pmg_kernel_resources.py.  The row-gather kernels share their cell walk and tile frame through function templates and
lambdas, and what such sharing can cost is registers: no kernel may fall below the occupancy it had before the walk and the
frame were shared (the figures below: that commit compiled with these flags), none may touch scratch memory or spill -- but for
the legacy matfree_cell<10> / <20>, which may not use more scratch than they did -- the static LDS is what it was, and the set of
kernel instantiations is the table's.  VGPR counts are printed, not asserted: within an occupancy step they may move."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel<template arguments>: (waves/SIMD, scratch bytes/lane, static LDS bytes) before the sharing
PARENT = {
    "asm_matrix_p1<1,1920,128>": (4, 0, 23168), "asm_matrix_p1<3,4096,256>": (3, 0, 49280), "asm_matrix_p1_node3<8704>": (1, 0, 73632),
    "asm_matrix_pk_pos<10,1,4>": (5, 0, 3216), "asm_matrix_pk_pos<20,1,4>": (5, 0, 3216),
    "asm_matrix_pk_pos<10,3,4>": (4, 0, 3216), "asm_matrix_pk_pos<20,3,8>": (4, 0, 3216),
    "asm_matrix_pk<10,1,4>": (4, 0, 2192), "asm_matrix_pk<20,1,8>": (4, 0, 2192),
    "asm_matrix_pk<10,3,4>": (3, 0, 2192), "asm_matrix_pk<20,3,8>": (3, 0, 2192),
    "asm_vector_p1<1>": (6, 0, 0), "asm_vector_p1<3>": (8, 0, 0),
    "asm_vector_pk<10,1>": (4, 0, 4000), "asm_vector_pk<10,3>": (7, 0, 800),
    "asm_vector_pk<20,1>": (3, 0, 16000), "asm_vector_pk<20,3>": (5, 0, 3200),
    "k_cell_geom<1>": (8, 0, 0), "k_cell_geom<3>": (8, 0, 0), "k_cell_load_p1<1>": (8, 0, 0), "k_cell_load_p1<3>": (8, 0, 0),
    "k_lift<4,1,1>": (7, 0, 0), "k_lift<4,3,1>": (5, 0, 0), "k_lift<10,1,2>": (6, 0, 4800), "k_lift<10,3,4>": (4, 0, 7200),
    "k_lift<20,1,4>": (6, 0, 19200), "k_lift<20,3,8>": (4, 0, 28800),
    "matfree_cell<4>": (8, 0, 0), "matfree_cell<10>": (1, 692, 4800), "matfree_cell<20>": (1, 772, 19200),
}
MAY_SPILL = ("matfree_cell<10>", "matfree_cell<20>")  # legacy: a thread holds a cell's whole element matrix row by row


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_assembly_kernels_keep_their_occupancy_and_stay_out_of_scratch(tmp_path):
    src = os.path.join(ROOT, "performance-test_amd", "csrc", "zzz_assemble.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fopenmp", "-I" + os.path.dirname(src),
           "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        # _ZN3zzz13asm_matrix_p1ILi1ELi1920ELi128EEEv...: the kernel and its integer template arguments
        m = re.match(r"_ZN3zzz\d+((?:asm_|k_cell_|k_lift(?!_)|matfree_cell)\w*?)I((?:Li\d+E)+)E", name)
        if not m:
            assert not re.match(r"_ZN3zzz\d+(asm_|k_cell_|k_liftI|matfree_cell)", name), name
            continue
        key = m.group(1) + "<" + ",".join(re.findall(r"Li(\d+)E", m.group(2))) + ">"
        num = {k: int(re.search(re.escape(k) + r": (\d+)", b).group(1))
               for k in ("VGPRs", "AGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
                         "LDS Size [bytes/block]")}
        print(key, num)
        assert key in PARENT, key
        occ, scratch, lds = PARENT[key]
        assert num["Occupancy [waves/SIMD]"] >= occ, (key, num)
        assert num["ScratchSize [bytes/lane]"] <= scratch, (key, num)
        if key not in MAY_SPILL:
            assert num["VGPRs Spill"] == 0 and num["SGPRs Spill"] == 0, (key, num)
        assert num["LDS Size [bytes/block]"] == lds, (key, num)
        seen.add(key)
    assert seen == set(PARENT), (sorted(seen - set(PARENT)), sorted(set(PARENT) - seen))
