"""The driver's --problem_type cgelasticity: elasticity's mesh, space, Dirichlet set and right-hand side on the matrix-free
operator of form a (no matrix), solved by linalg::cg as cgpoisson is (default) or, --cg_solver ksp, by KSPCG with the options
database; what the matrix-free operator declines is refused before any GPU work, with the reason."""
import subprocess

from _gpu_helpers import *  # noqa: F401,F403 -- np / os / zzz / pytest

pytestmark = pytest.mark.gpu  # noqa: F405

EXE = os.path.join(zzz.PKG, "dolfinx-scaling-test")
SIZE = ["--ndofs", "30000", "--order", "2"]
KSP = ["-pc_type", "jacobi", "-ksp_rtol", "1e-8"]


def _run(args):
    o = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stderr[-1000:]
    return (int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]),
            float(o.stdout.split("*** Solution norm:  ")[1].split()[0]), o.stdout)


def test_default_mode_runs_linalg_cg():
    its, nrm, s = _run(["--problem_type", "cgelasticity"] + SIZE)
    print(s[-1500:])
    assert "CG matrix-free action processed: " in s and "Gdof/s" in s and "ZZZ Solve" in s
    assert "  Problem type:    cgelasticity" in s and "ZZZ Assemble matrix" not in s and "ZZZ Assemble vector" in s
    assert 0 < its <= 100 and nrm > 0


@pytest.mark.parametrize("ranks", [[], ["--ngpus", "2", "--comm", "local"]], ids=["one-rank", "two-ranks"])
def test_cg_solver_ksp_against_the_assembled_elasticity_run(ranks):
    its_a, nrm_a, _ = _run(["--problem_type", "elasticity"] + SIZE + KSP + ranks)
    its_m, nrm_m, s = _run(["--problem_type", "cgelasticity", "--cg_solver", "ksp", "-ksp_view"] + SIZE + KSP + ranks)
    print(f"assembled {its_a} iterations, |u| {nrm_a}; matrix-free {its_m} iterations, |u| {nrm_m}")
    assert abs(its_m - its_a) <= 2
    assert abs(nrm_m - nrm_a) <= 1e-6 * nrm_a
    assert "type=shell" in s and "ZZZ Assemble matrix" not in s


def test_refusals_say_why():
    for bad, word in ((["--scalar_type", "float32"], "float32"), (["-pc_type", "chebyshev_jacobi"], "-pc_type"),
                      (["-pc_type", "mg"], "-pc_type"), (["-pc_type", "pmg"], "-pc_type"), (["-ksp_type", "pipecg"], "pipecg"),
                      (["-ksp_cg_single_reduction"], "single_reduction"), (["--operator", "matfree"], "already matrix-free"),
                      (["--cg_solver", "gmres"], "linalg or ksp")):
        o = subprocess.run([EXE, "--problem_type", "cgelasticity"] + SIZE + bad, capture_output=True, text=True, timeout=60)
        assert o.returncode != 0 and word in o.stderr, (bad, o.stderr[-500:])
        assert "Test problem summary" not in o.stdout
    # --cg_solver belongs to cgelasticity; the unknown-problem message names it; --operator matfree keeps refusing elasticity
    for args, word in ((["--problem_type", "poisson", "--cg_solver", "ksp"], "cgelasticity only"),
                       (["--problem_type", "stokes"], "cgelasticity"),
                       (["--problem_type", "elasticity", "--operator", "matfree"], "cgelasticity")):
        o = subprocess.run([EXE] + args + SIZE, capture_output=True, text=True, timeout=60)
        assert o.returncode != 0 and word in o.stderr, (args, o.stderr[-500:])
