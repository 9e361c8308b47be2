"""Build-time guard for the direction kernels of the classical CG loop (csrc/zzz_cg.hip), in the manner of
tests/test_kernel_resources.py: k_update_p in place and its two forms with the solution update deferred (k_update_p_light,
k_update_p_flush<.., K>), plus the pass that applies what is pending when a solve ends (k_x_apply_pending<K>).  They are
bound by HBM bytes, so what matters is that none of them touches scratch memory, and that neither deferred form runs at
a lower occupancy than the in-place kernel the headline ran with until now, k_update_p<true, 1>, in the same compile
(the flush form holds K alphas and reads K - 1 more vectors per entry)."""
import os

import pytest

from _kernel_resources import HIPCC, kernel_resources, template_args


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_direction_kernels_have_no_scratch_and_keep_the_in_place_occupancy():
    found = {}
    for name, k in kernel_resources("zzz_cg.hip").items():
        key = template_args(name)
        if not key or key[0] not in ("k_update_p", "k_update_p_light", "k_update_p_flush", "k_x_apply_pending"):
            continue
        print(*key, k)
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (name, k)
        found[key] = k["occ"]
    flags = [(nt, dz) for nt in (0, 1) for dz in (0, 1, 2)]
    # every instantiation the solver can launch is there: load policy x (inverse diagonal as doubles | 16-bit | 8-bit codes) [x K]
    assert {k for k in found if k[0] == "k_update_p"} == {("k_update_p", f) for f in flags}
    assert {k for k in found if k[0] == "k_update_p_light"} == {("k_update_p_light", f) for f in flags}
    assert {k for k in found if k[0] == "k_update_p_flush"} == {("k_update_p_flush", f + (K,)) for f in flags for K in (2, 4, 8)}
    assert {k for k in found if k[0] == "k_x_apply_pending"} == {("k_x_apply_pending", (K,)) for K in (2, 4, 8)}
    base = found[("k_update_p", (1, 1))]
    for (kern, args), occ in found.items():
        if kern in ("k_update_p_light", "k_update_p_flush"):
            assert occ >= base, (kern, args, occ, base)
