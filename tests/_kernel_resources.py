"""What the tests/test_*kernel_resources.py modules share: one cross-compile of a source under csrc/ for gfx950 per process, and
the compiler's resource remarks of that compile per mangled function name.  Nothing here reads instruction text."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

_FIELDS = {"vgprs": r"VGPRs: (\d+)", "agprs": r"AGPRs: (\d+)", "sgprs": r"TotalSGPRs: (\d+)", "occ": r"Occupancy \[waves/SIMD\]: (\d+)",
           "scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "vspill": r"VGPRs Spill: (\d+)", "sspill": r"SGPRs Spill: (\d+)",
           "lds": r"LDS Size \[bytes/block\]: (\d+)"}
_cache = {}


def kernel_resources(src_name):
    """{mangled function name: {vgprs, agprs, sgprs (total), occ (waves/SIMD), scratch (bytes/lane), vspill, sspill, lds
    (bytes/block)}} of performance-test_amd/csrc/<src_name>; compiled at the first call, the same dictionary afterwards."""
    if src_name not in _cache:
        csrc = os.path.join(ROOT, "performance-test_amd", "csrc")
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + csrc,
                   "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "performance-test_amd", "host"), "-c",
                   os.path.join(csrc, src_name), "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        # remarks come in blocks: "Function Name: <mangled>" followed by the resource lines of that function
        _cache[src_name] = {b.split()[0]: {k: int(re.search(p, b).group(1)) for k, p in _FIELDS.items()}
                            for b in re.split(r"remark: Function Name: ", r.stderr)[1:]}
    return _cache[src_name]


def template_args(mangled):
    """_ZN3zzz<len><name>I<L[bi]<value>E ...>EE... -> (name, (values as int, ...)); None for any other name."""
    m = re.match(r"_ZN3zzz(\d+)", mangled)
    if not m:
        return None
    name, rest = mangled[m.end():m.end() + int(m.group(1))], mangled[m.end() + int(m.group(1)):]
    a = re.match(r"I((?:L[bi]\d+E)+)EE", rest)
    return (name, tuple(int(v) for v in re.findall(r"L[bi](\d+)E", a.group(1)))) if a else None
