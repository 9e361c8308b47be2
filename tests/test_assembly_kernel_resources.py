"""Build-time guard for the assembly kernels (csrc/zzz_assemble.hip with csrc/zzz_asm_elem.h), in the manner of
tests/test_pmg_kernel_resources.py.  The row-gather kernels share their cell walk and tile frame through function templates and
lambdas, and what such sharing can cost is registers: no kernel may fall below the occupancy it had before the walk and the
frame were shared (the figures below: that commit compiled with these flags), none may touch scratch memory or spill -- but for
the legacy matfree_cell<10> / <20>, which may not use more scratch than they did -- the static LDS is what it was, and the set of
kernel instantiations is the table's.  VGPR counts are printed, not asserted: within an occupancy step they may move."""
import os
import re

import pytest

from _kernel_resources import HIPCC, kernel_resources

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
def test_assembly_kernels_keep_their_occupancy_and_stay_out_of_scratch():
    seen = set()
    for name, num in kernel_resources("zzz_assemble.hip").items():
        # _ZN3zzz13asm_matrix_p1ILi1ELi1920ELi128EEEv...: the kernel and its integer template arguments
        m = re.match(r"_ZN3zzz\d+((?:asm_|k_cell_|k_lift(?!_)|matfree_cell)\w*?)I((?:Li\d+E)+)E", name)
        if not m:
            assert not re.match(r"_ZN3zzz\d+(asm_|k_cell_|k_liftI|matfree_cell)", name), name
            continue
        key = m.group(1) + "<" + ",".join(re.findall(r"Li(\d+)E", m.group(2))) + ">"
        print(key, num)
        assert key in PARENT, key
        occ, scratch, lds = PARENT[key]
        assert num["occ"] >= occ, (key, num)
        assert num["scratch"] <= scratch, (key, num)
        if key not in MAY_SPILL:
            assert num["vspill"] == 0 and num["sspill"] == 0, (key, num)
        assert num["lds"] == lds, (key, num)
        seen.add(key)
    assert seen == set(PARENT), (sorted(seen - set(PARENT)), sorted(set(PARENT) - seen))
