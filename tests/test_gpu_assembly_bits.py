"""GPU parity tests: the row-gather assembly kernels (csrc/zzz_assemble.hip, csrc/zzz_asm_elem.h) keep every bit.

SHA-256 digests of the raw bytes of the assembled CSR values, of b, of b after the lifting pass (k_lift, k_bc_set_values) on
seeded noise for u0, and -- Poisson -- of the two-pass matrix-free action (ZZZ_MF_LEGACY=1: matfree_cell) on a seeded vector,
against tests/golden/assembly_bits.json.  The digests there were recorded on an MI355X from the library of the commit that
file names (the last one before the kernels' cell walk and tile frame were shared), so a change to these kernels that moves a
bit of any case fails here by name.  The cases are the smallest shapes at which a walk or a frame can go wrong: a cube with
single-cell rows, one with odd and even cell counts (the two-per-turn loop and its tail), one that spans many tiles, and the
unstructured mesh for irregular valences; P2 / P3 with the stored positions and with ZZZ_ASM_SEARCH=1, elasticity P1 by node
and by scalar row (ZZZ_ASM_NODE3).

Recording (with another build selected by ZZZ_HIP_LIB):  python tests/test_gpu_assembly_bits.py --record --commit <hash>"""
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "performance-test_amd"), os.path.join(_root, "oracle")]

from _gpu_helpers import *  # noqa: F401,F403,E402 -- np / os / pytest / zzz

GOLDEN = os.path.join(GOLD, "assembly_bits.json")  # noqa: F405
PAIRS = [(p, o) for p in ("poisson", "elasticity") for o in (1, 2, 3)]
MANY_TILES = {("poisson", 1): (12, 11, 13), ("elasticity", 1): (12, 11, 13), ("poisson", 2): (6, 5, 7), ("poisson", 3): (6, 5, 7),
              ("elasticity", 2): (5, 4, 6), ("elasticity", 3): (3, 4, 3)}
MESHES = ([(p, o, ("cube", d)) for d in ((1, 1, 1), (3, 2, 4)) for p, o in PAIRS]
          + [(p, o, ("cube", MANY_TILES[p, o])) for p, o in PAIRS]
          + [("poisson", 1, ("spoke", 3)), ("poisson", 2, ("spoke", 2))])


def _variants(problem, order):
    """the environment of every matrix kernel that serves (problem, order)"""
    if order > 1:
        return [{}, {"ZZZ_ASM_SEARCH": "1"}]
    return [{"ZZZ_ASM_NODE3": "1"}, {"ZZZ_ASM_NODE3": "0"}] if problem == "elasticity" else [{}]


CASES_BITS = [(p, o, mesh, env) for p, o, mesh in MESHES for env in _variants(p, o)]


def _case_id(case):
    p, o, (kind, size), env = case
    mesh = f"spoke{size}" if kind == "spoke" else "cube" + "x".join(str(n) for n in size)
    return "-".join([p, f"P{o}", mesh] + [f"{k}={v}" for k, v in env.items()])


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _noise_values(P, seed):
    """as _noise_values of tests/test_gpu_lifting.py: seeded noise at every dof, NaN at a handful of unconstrained entries"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P.nloc * P.bs)
    free = np.nonzero(P.bc_marker() == 0)[0]
    g[rng.choice(free, size=min(7, free.size), replace=False)] = np.nan
    return g


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _digests(case):
    problem, order, (kind, size), env = case
    P = zzz.Part.spoke(problem, order, size) if kind == "spoke" else zzz.Part(problem, order, *size)
    out = {}
    with _Env(env):
        with zzz.Context(0) as c:
            c.upload_part(P)
            c.pattern_build()
            c.assemble_matrix(P.form)
            out["A"] = _sha(c.csr_download()[2])
            c.assemble_vector(P.form)
            out["b"] = _sha(c.vec_download(zzz.VEC_B))
            c.upload_bc_values(_noise_values(P, 11 * order + P.bs))
            c.assemble_vector(P.form)
            out["b_lifted"] = _sha(c.vec_download(zzz.VEC_B))
            if P.bs == 1:
                xv = np.random.default_rng(7 + order).standard_normal(P.n_owned)
                with _Env({"ZZZ_MF_LEGACY": "1"}):
                    out["action_legacy"] = _sha(c.action(xv))
    return out


@pytest.mark.gpu  # noqa: F405
@pytest.mark.parametrize("case", CASES_BITS, ids=_case_id)  # noqa: F405
def test_assembly_keeps_the_recorded_bits(case):
    with open(GOLDEN) as f:
        gold = json.load(f)
    cid = _case_id(case)
    assert cid in gold["digests"], f"{cid}: no recorded digests"
    got, want = _digests(case), gold["digests"][cid]
    assert sorted(got) == sorted(want), (cid, sorted(got), sorted(want))
    for name in ("A", "b", "b_lifted", "action_legacy"):
        if name in want:
            assert got[name] == want[name], f"{cid}: {name} differs from the values of commit {gold['commit']}"


def test_every_recorded_case_is_run():
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold["digests"]) == sorted(_case_id(c) for c in CASES_BITS)


def _record(argv):
    import shutil
    import subprocess

    commit = argv[argv.index("--commit") + 1]
    out = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    hipcc = subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    rec = {"commit": commit, "hipcc": next((ln for ln in hipcc if "HIP version" in ln), ""), "digests": {}}
    for case in CASES_BITS:
        rec["digests"][_case_id(case)] = _digests(case)
        print(_case_id(case), rec["digests"][_case_id(case)]["A"][:16], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    assert "--record" in sys.argv and "--commit" in sys.argv, __doc__
    _record(sys.argv)
