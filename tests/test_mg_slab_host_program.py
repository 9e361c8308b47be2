"""csrc/zzz_mg_transfer.h on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer: what the transfer kernels of
ZZZ_PC_MG (csrc/zzz_mg.hip) share with host code is host-compilable, and tools/mg_slab_host.cpp (a stand-alone program with its
own main) runs the two walks on the whole cube and on every z-slab of a partition, each slab with vectors of exactly its own
length.  The program checks that the slabs' prolongation is the whole walk's bit for bit, that a slab writes only the coarse
planes it says it reaches and that the rank-ordered sum of the partial restrictions stays within 1e-13 of max |out| of the whole
one; this test also reads the vectors it wrote and holds them against the scipy restatement of the transfer (tests/_mg_ref.py)
at the same bar -- test_gpu_mg's transfer bar: a sum of at most about 30 terms, which rounding cannot reach."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CLANG = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "lib", "llvm", "bin", "clang++")

CASES = [(1, (10, 9, 12), 2), (1, (10, 9, 12), 3), (1, (10, 9, 12), 4), (1, (7, 6, 9), 3), (1, (6, 5, 3), 3), (3, (5, 5, 8), 2),
         (3, (5, 5, 8), 4)]


def _masked_p(bs, n):
    from _mg_ref import prolongation
    import scipy.sparse as sp

    def free(d):
        px, py, pz = (v + 1 for v in d)
        ix, iy = np.arange(px * py * pz) % px, (np.arange(px * py * pz) // px) % py
        on = (ix == 0) | (ix == d[0]) if bs == 1 else iy == 0
        return sp.diags(np.repeat(1.0 - on.astype(float), bs))

    nc = tuple(max(2, (v + 1) // 2) for v in n)
    return (free(n) @ prolongation(n, nc, bs) @ free(nc)).tocsr()


def test_host_program_under_sanitizers(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm's clang++ not available")
    exe = str(tmp_path / "mg_slab_host")
    src = os.path.join(ROOT, "performance-test_amd", "tools", "mg_slab_host.cpp")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "performance-test_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]  # (a sanitizer report goes to stderr and ends the run)
    assert r.stdout.count("case ") == len(CASES) and r.stdout.strip().endswith("ok")
    for k, (bs, n, nparts) in enumerate(CASES):
        raw = np.fromfile(str(tmp_path / f"case_{k}.bin"), np.int64, 7)
        assert tuple(raw[:5]) == (bs,) + n + (nparts,)
        nf, nc = int(raw[5]), int(raw[6])
        v = np.fromfile(str(tmp_path / f"case_{k}.bin"), np.float64, offset=56)
        assert v.size == 3 * nc + 2 * nf
        e, r_, pe, rsum, rt = np.split(v, [nc, nc + nf, nc + 2 * nf, 2 * nc + 2 * nf])
        P = _masked_p(bs, n)
        assert P.shape == (nf, nc)
        d0 = np.abs(pe - P @ e).max() / np.abs(pe).max()
        d1 = np.abs(rsum - P.T @ r_).max() / np.abs(rt).max()
        d2 = np.abs(rt - P.T @ r_).max() / np.abs(rt).max()
        print(f"case {k}: prolongation {d0:.2e}, rank-ordered restriction {d1:.2e}, whole restriction {d2:.2e} of max |out|")
        assert d0 <= 1e-13 and d1 <= 1e-13 and d2 <= 1e-13
