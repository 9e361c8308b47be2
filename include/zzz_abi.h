/*
 * zzz_abi.h -- C-ABI of libzzz_hip.so: the MI355X (gfx950) implementation of the hot path of
 * FEniCS/performance-test (`ZZZ Assemble matrix`, `ZZZ Assemble vector`, `ZZZ Solve`).
 *
 * Plain C, POD arguments, opaque context handle.  No exceptions cross this boundary: every
 * function returns 0 on success or a ZZZ_ERR_* code; zzz_last_error() gives the message.
 * The host owns host arrays; every upload copies; the library owns all device memory behind the
 * context; downloads write into caller-provided buffers.  One driving host thread per context;
 * one context per GPU (one process or thread per GPU).  Work is enqueued asynchronously on the
 * context's HIP stream except the *_download functions, zzz_sync and zzz_cg_solve.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository, FEniCS/performance-test @ 2025-10-24).
 *
 * Data model at the boundary (one mesh partition = one context, DOLFINx's per-rank view):
 *   - block dofs [0, n_owned) are owned, [n_owned, n_owned + n_ghost) are ghosts
 *     (the la::Vector layout, src/cgpoisson_problem.cpp:212-215); scalar dof = bs*block + comp.
 *   - the partition holds every cell that touches an owned dof (one ghost-cell layer), so each
 *     owned matrix row and vector entry is complete locally and MatAssemblyBegin/End's row
 *     exchange (src/poisson_problem.cpp:132-133) and b.scatter_rev (:154) have nothing to ship.
 *   - cell_dofs follows the Basix local ordering of the P_k gll_warped tetrahedron
 *     (src/poisson_problem.cpp:35-38): vertices 0-3; edges e0=(2,3) e1=(1,3) e2=(1,2) e3=(0,3)
 *     e4=(0,2) e5=(0,1), k-1 dofs each, counted from the edge's first local vertex; faces
 *     f0=(1,2,3) f1=(0,2,3) f2=(0,1,3) f3=(0,1,2).  Edge orientation is resolved by the dofmap
 *     (the caller permutes an edge's sub-dofs when the global direction opposes the local one),
 *     so the kernels apply no dof transformation -- DOLFINx's convention for Lagrange.
 *   - the matrix is scalar CSR (PETSc AIJ): fp64 values, int32 columns (local scalar indices,
 *     ascending within a row), int32 row pointers; rows = owned scalar dofs.
 */
#ifndef ZZZ_ABI_H
#define ZZZ_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zzz_ctx zzz_ctx;

/* error classes */
enum
{
  ZZZ_OK = 0,
  ZZZ_ERR_ARG = 1,     /* bad argument / call order (std::runtime_error in the reference) */
  ZZZ_ERR_HIP = 2,     /* HIP runtime error */
  ZZZ_ERR_RCCL = 3,    /* RCCL error / librccl not loadable */
  ZZZ_ERR_NO_GPU = 4,  /* no usable device: the library has no CPU fallback */
  ZZZ_ERR_LIMIT = 5,   /* size exceeds an int32 index range */
  ZZZ_ERR_DIVERGED = 6 /* the solve did not converge AND zzz_solver_opts.error_if_not_converged was set */
};

/* forms: form_Poisson_{a,L,M}{1,2,3}, form_Elasticity_{a,L}{1,2,3}
 * (src/poisson_problem.cpp:110-119, src/elasticity_problem.cpp:184-191) */
enum
{
  ZZZ_FORM_POISSON = 0,
  ZZZ_FORM_ELASTICITY = 1
};

enum
{
  ZZZ_COEFF_F = 0, /* "w0" of L (src/poisson_problem.cpp:117, src/elasticity_problem.cpp:189) */
  ZZZ_COEFF_G = 1  /* "w1" of the Poisson L (src/poisson_problem.cpp:117) */
};

enum
{
  ZZZ_VEC_B = 0, /* right-hand side b */
  ZZZ_VEC_U = 1  /* solution u (u->x() of the reference) */
};

/* Krylov options: what "-ksp_type cg -pc_type jacobi -ksp_rtol 1e-8" selects through
 * solver.set_from_options() (src/poisson_problem.cpp:169), or the arguments of linalg::cg
 * (src/cg.h:39-40). */
enum
{
  ZZZ_PC_NONE = 0,
  ZZZ_PC_JACOBI = 1,
  /* polynomial preconditioner: z = p_k(D^-1 A) D^-1 r, k steps of the Chebyshev iteration for D^-1 A started from zero
   * (PETSc: -pc_type ksp -ksp_ksp_type chebyshev -ksp_ksp_max_it k -ksp_pc_type jacobi [EXT]).  The "stronger
   * preconditioner" of README.md:61-62,108-110 that needs only the product and no reduction inside its application:
   * fewer CG iterations, i.e. fewer all-reduces per solve, for more products -- for multi-GPU runs.  Spectrum
   * bounds [hi / pc_ratio, hi] with hi = min(Gershgorin's bound of D^-1 A, 1.1 x a Lanczos estimate: pc_esteig_its).
   * ZZZ_CG_PETSC + ZZZ_OP_CSR only (classical or single-reduction form). */
  ZZZ_PC_CHEBYSHEV_JACOBI = 2,
  /* geometric multigrid: one V-cycle per application (PCSetUp / PCApply of PETSc's PCMG behind
   * solver.set_from_options(), src/poisson_problem.cpp:169; the reference's README.md:59-146 runs every recommended
   * configuration with a multigrid preconditioner, GAMG or BoomerAMG -- this is the geometric counterpart for its own
   * cube meshes, not an algebraic one).  Scope: P1, Poisson and elasticity, a context whose feed came from
   * zzz_cube_generate with nparts == 1, the assembled operator, ZZZ_CG_PETSC in its classical form, all three norm
   * types.  Declined with ZZZ_ERR_ARG and a message that names the reason (the context stays usable): order 2 or 3,
   * an uploaded / unstructured feed, a communicator attached (but see SEVERAL RANKS below), ZZZ_OP_MATFREE,
   * single_reduction, ZZZ_CG_PIPE, ZZZ_CG_CGH.
   * Level l+1 is the same problem RE-DISCRETISED on max(2, (n+1)/2) cells per axis (not nested when n is odd), generated,
   * patterned and assembled by the library's own kernels; the coarsest level is the first with at most
   * pc_mg_coarse_eq_limit scalar dofs (or 2 x 2 x 2 cells, or level pc_mg_levels, 12 at most) and is solved with a dense
   * inverse (at most 4 096 dofs).  Transfer: the coarse Kuhn-P1 function evaluated at the fine vertices, closed form, no
   * P stored, constrained dofs zeroed on both sides.  Smoother: pc_degree steps of Chebyshev-Jacobi on
   * [hi / pc_ratio, hi] before (from zero) and after (from the corrected iterate) -- the same polynomial, so the cycle is
   * symmetric; for mg pc_degree == 0 selects 2 and pc_ratio <= 1 selects 10; hi is each level's own bound, taken as
   * ZZZ_PC_CHEBYSHEV_JACOBI takes it (pc_esteig_its).  The hierarchy is built by the first solve (or zzz_mg_setup), kept
   * across solves, rebuilt when the feed changes, its values refreshed when the matrix values change.  After
   * zzz_csr_upload_values on the context the coarse levels STAY the re-discretised ones of the generated problem.
   * SEVERAL RANKS: a communicator of two or more ranks with a transport (zzz_comm_init or zzz_comm_init_local) on a cube
   * generated by zzz_cube_generate(..., nparts = nranks, part = rank) is served too.  Level 0 stays on the z-slabs (its
   * products exchange the halo, its bound is the ranks' common one, as ZZZ_PC_CHEBYSHEV_JACOBI has them) and EVERY coarser
   * level is held whole by every rank, built by the level rule from the global cube: the one-rank hierarchy and, up to the
   * order of one sum, the one-rank preconditioner, whatever the number of ranks.  The prolongation reads the whole level-1
   * vector and writes the owned fine dofs, with the one-rank kernel's bits; the restriction leaves each rank's partial sums
   * over its own fine vertex planes in the whole level-1 vector, zero where it reaches nothing, and the communicator adds
   * them (one all-reduce of the level-1 right-hand side per cycle, in the communicator's order).  From level 1 down every
   * rank runs the same cycle on the same numbers.  zzz_mg_setup, zzz_mg_apply, zzz_mg_transfer at level 0 (both directions)
   * and zzz_cg_solve with this preconditioner are then COLLECTIVE; before a set-up returns on any rank the ranks agree on
   * its status, so none enters a cycle while another has failed.  Declined there, with ZZZ_ERR_ARG and the reason: a
   * communicator of ONE rank (as before: "a communicator is attached"), a peer-only communicator (zzz_comm_init_peer_only:
   * the all-reduce needs a transport), a cube generated as another part or of another number of parts than the
   * communicator's rank and size, an uploaded feed (the native partition behind zzz_ghost_layer_build is one), a cube under
   * the coarse limit (one level: a dense solve of a matrix no rank holds).  ZZZ_PC_PMG, ZZZ_PC_AGG, ZZZ_PC_SAGG and
   * ZZZ_PC_SAGG_RBM keep declining any communicator. */
  ZZZ_PC_MG = 3,
  /* p-multigrid for orders 2 and 3 on the same cubes: ZZZ_PC_MG's scope with the order test dropped.  Level 0 is the
   * caller's Pk matrix, smoothed like every other level; level 1 is the SAME cube re-discretised at order 1 (generated,
   * patterned and assembled like ZZZ_PC_MG's coarse levels); levels 2.. are ZZZ_PC_MG's hierarchy of that P1 problem, to
   * which pc_mg_coarse_eq_limit and the dense-size rule apply.  pc_mg_levels counts all levels, so at order > 1 a value
   * of 1 is declined.  Transfer between levels 0 and 1: the P1 function evaluated at the Pk dof points of the Kuhn cube
   * (1 term at a vertex, 2 on an edge with the weights of the Pk nodes, 3 x 1/3 at a face centroid), closed form, no P
   * stored, fixed summation order, constrained dofs zeroed on both sides.  At order 1 it builds exactly ZZZ_PC_MG's
   * hierarchy.  ZZZ_PC_MG itself keeps declining orders 2 and 3. */
  ZZZ_PC_PMG = 4,
  /* Unsmoothed (plain) aggregation multigrid from the assembled matrix alone (PETSc: -pc_type gamg
   * -pc_gamg_agg_nsmooths 0).  Served: any context with a sparsity pattern and matrix values -- generated, uploaded,
   * unstructured or zzz_csr_upload_values feeds, block size 1 and 3, orders 1 to 3 -- with ZZZ_OP_CSR, ZZZ_CG_PETSC in its
   * classical form, all three norm types, one rank.  Declined with ZZZ_ERR_ARG and the reason (the context stays usable):
   * a communicator attached, ZZZ_OP_MATFREE, single_reduction, ZZZ_CG_PIPE, ZZZ_CG_CGH.  Per level: the block dofs with an
   * unconstrained component are the nodes of a graph (adjacent: a nonzero scalar entry in their coupling); the roots
   * are a distance-2 maximal independent set chosen in synchronous rounds by a fixed integer priority (csrc/zzz_agg.hip
   * gives the formula), two joining rounds attach the rest, what is left becomes singletons.  P is 1 from each
   * unconstrained scalar dof to the same component of its aggregate (piecewise constant, never stored; no rigid-body
   * modes), the coarse matrix is P^T A P summed in one fixed order, built on the device; coarse levels have no Dirichlet
   * rows.  Levels are added until one has at most pc_mg_coarse_eq_limit scalar dofs (0: 1000), pc_mg_levels is reached,
   * there are 12, or an aggregation reduces the dofs by less than a factor of 2; the last one is solved with the dense
   * inverse (at most 4 096 dofs, else declined).  Smoother, cycle and options (pc_degree, pc_ratio, pc_esteig_its) are
   * ZZZ_PC_MG's.  The hierarchy is kept while pattern and Dirichlet set are kept; new matrix values refresh the coarse
   * VALUES on the kept aggregates. */
  ZZZ_PC_AGG = 5,
  /* Smoothed-aggregation multigrid: ZZZ_PC_AGG with one prolongator-smoothing step (PETSc: -pc_type gamg
   * -pc_gamg_agg_nsmooths 1, no near-nullspace).  Scope, refusals, options, level rule, smoother, cycle and dense coarsest
   * solve are ZZZ_PC_AGG's, word for word.  Per level (csrc/zzz_sagg.hip; every sum a chain of plain double additions of
   * individually rounded products, in ascending index -- of the caller's numbering on level 0, of the level's own below):
   * the aggregates are ZZZ_PC_AGG's rule on the graph of that level's matrix (the coarse matrices are denser here, so the
   * coarse aggregates differ from ZZZ_PC_AGG's; level 0's are the same); P_t is ZZZ_PC_AGG's P; omega = 4 / (3 hi) with hi
   * the bound of D^-1 A that the level's smoother uses (pc_esteig_its), so a level's bound comes before the next level's
   * values; P = (I - omega D^-1 A) P_t is STORED as CSR with ascending coarse columns -- pattern: (i, J) wherever row i is
   * unconstrained and has a structural entry a_ik, zero or not, with k unconstrained and mapped to J by P_t; value:
   * s = sum_k a_ik over those k, P(i, J) = delta - (omega s) / a_ii with delta = 1 when P_t(i, J) = 1, else 0; rows of
   * constrained dofs are empty -- and so is R = P^T, coarse rows with ascending fine index, so the restriction is a gather
   * summed in one fixed order (64 interleaved partial sums front to back, then a shuffle tree); T = A P, T(i, J) = sum_k a_ik P(k, J); A_c = P^T T, A_c(I, J) = sum_i P(i, I) T(i, J), its
   * pattern every (I, J) that receives a structural term, adopted by the coarse level as ZZZ_PC_AGG's (block size kept, no
   * Dirichlet rows).  A level whose products have more terms than 32-bit positions take is declined with ZZZ_ERR_LIMIT.
   * The hierarchy is kept while pattern and Dirichlet set are kept; new matrix values (or another pc_esteig_its) refresh
   * the bounds and the values of P and of the coarse matrices level by level, to the bits of a fresh set-up. */
  ZZZ_PC_SAGG = 6,
  /* ZZZ_PC_SAGG with a tentative prolongator that carries the near-nullspace -- the six rigid-body modes of
   * zzz_near_nullspace_build -- through every level (PETSc: -pc_type gamg with MatSetNearNullSpace, what the reference builds
   * the modes for).  Declined with ZZZ_ERR_ARG: everything ZZZ_PC_AGG declines; block size != 3 (for scalar problems use
   * -pc_type sagg); a context with no near-nullspace built (zzz_near_nullspace_build, after the last dofmap upload).
   * ZZZ_PC_SAGG itself never reads the modes.  The rule, per level (csrc/zzz_sagg_rbm.hip).  Scope, options, level rule,
   * smoother, cycle, spectrum bound and omega = 4 / (3 hi) are ZZZ_PC_SAGG's.  Every sum is a chain of plain double additions
   * of individually rounded products, with no fused multiply-add.
   *   node size   3 on level 0, 6 on every coarse level.
   *   B           level 0: the library's six vectors as zzz_near_nullspace_build left them, in the caller's numbering, entries
   *               of constrained scalar dofs taken as 0.  Level l + 1: the B_c below, 6 columns by 6 rows per aggregate.
   *   aggregates  ZZZ_PC_AGG's rule on the node graph of the level's matrix: nodes are blocks of 3 scalar dofs on level 0 and
   *               blocks of 6 below.
   *   P_t, B_c    per aggregate J, its m member nodes in ascending index (the caller's numbering on level 0): take the rows of
   *               B of its member dofs, node-major then component ascending; modified Gram-Schmidt over the six columns in
   *               column order q = 0..5: for j < q, R(j, q) = <Q_j, b_q>, then b_q -= R(j, q) Q_j; then R(q, q) = |b_q| and
   *               Q_q = b_q / R(q, q).  A column is DROPPED when |b_q| after the projections is at most 2^-30 of its norm
   *               before them, or when it is zero: then Q_q = 0 and row q of R is 0.  P_t(row, (J, q)) = Q_q(row); rows of
   *               constrained dofs and dropped columns carry no entries.  B_c's rows (J, 0..5) are R.
   *   one sum     every inner product and norm: partial sum l (l = 0..63) adds the products of the rows l, l + 64, ... front
   *               to back, then the 64 partial sums meet in the tree s[i] += s[i + o] for i < o, o = 32, 16, 8, 4, 2, 1; the
   *               result is s[0].  A norm is the square root of that sum of squares.
   *   P           P_t - omega D^-1 (A P_t): P(i, (J, q)) = P_t(i, (J, q)) - (omega s) / a_ii, s = sum_k a_ik P_t(k, (J, q))
   *               over the unconstrained k in ascending k.  Pattern: (i, (J, q)) wherever row i is unconstrained and has a
   *               structural a_ik with k unconstrained, k in aggregate J and column q kept.  Rows of constrained dofs are empty.
   *   R, T, A_c   R = P^T, T = A P and A_c = P^T T exactly as ZZZ_PC_SAGG forms them: sorted term lists, ascending summation
   *               index, one thread per run.
   *   dropped     a dropped coarse dof (J, q) has no entry in P; its row of A_c is the single entry 1 on the diagonal.  On the
   *               next level it is an ordinary dof with a zero row in B.
   * The coarse levels are scalar matrices (the node size belongs to the level).  The aggregates, Q, B_c and the drops depend
   * on B, the Dirichlet bytes and the kept aggregates only: new matrix values (or another pc_esteig_its) re-form the values of
   * P, T and A_c on the kept lists, to the bits of a fresh set-up.  P has six columns per aggregate: the ZZZ_ERR_LIMIT of
   * 32-bit term positions comes much earlier than ZZZ_PC_SAGG's, near 1.7 M dofs on generated P1 elasticity cubes. */
  ZZZ_PC_SAGG_RBM = 7
};
enum
{
  ZZZ_NORM_PRECONDITIONED = 0, /* PETSc KSPCG default: ||M^-1 r|| */
  ZZZ_NORM_UNPRECONDITIONED = 1,
  ZZZ_NORM_NATURAL = 2
};
enum
{
  ZZZ_CG_PETSC = 0, /* KSPCG: zero initial guess, test dp <= max(rtol*dp0, atol) */
  ZZZ_CG_CGH = 1,   /* src/cg.h:38-86: x is the initial guess, test <r,r>/<r0,r0> < rtol^2 */
  /* [EXT] KSPPIPECG, what solver.set_from_options() selects for -ksp_type pipecg (Ghysels & Vanroose 2014, Alg. 4):
   * the iteration of ZZZ_CG_PETSC with r, u = M^-1 r, w = A u and their directions kept by recurrence, so that the
   * ONE fused reduction of (<r,u>, <w,u>, norm) of an iteration overlaps its product n = A M^-1 w instead of
   * standing in front of it; two launches per iteration.  Conventions (zero initial guess, KSPConvergedDefault,
   * norm types, history, reasons) as ZZZ_CG_PETSC.  ZZZ_OP_CSR with ZZZ_PC_NONE | ZZZ_PC_JACOBI only, and not with
   * single_reduction.  No multi-GPU hardware run of this form exists. */
  ZZZ_CG_PIPE = 2
};
enum
{
  ZZZ_OP_CSR = 0,    /* assembled operator (poisson, elasticity) */
  ZZZ_OP_MATFREE = 1 /* cgpoisson's action(a, un) (src/cgpoisson_problem.cpp:193-230); on a context of block size 3 the same
                        for form a of src/Elasticity.py (the driver's cgelasticity).  At either block size: ZZZ_CG_CGH with
                        ZZZ_PC_NONE, ZZZ_CG_PETSC with ZZZ_PC_NONE or ZZZ_PC_JACOBI and any norm type, with or without a
                        communicator; declined: Chebyshev-Jacobi, mg, pmg, single_reduction, ZZZ_CG_PIPE */
};

typedef struct
{
  int32_t variant;  /* ZZZ_CG_PETSC | ZZZ_CG_CGH | ZZZ_CG_PIPE */
  int32_t pc;       /* ZZZ_PC_* (ZZZ_CG_CGH requires ZZZ_PC_NONE; with ZZZ_OP_MATFREE: none or jacobi) */
  int32_t norm;     /* ZZZ_NORM_* (ZZZ_CG_PETSC only) */
  int32_t op;       /* ZZZ_OP_* */
  int32_t max_it;   /* -ksp_max_it (PETSc default 10000) / kmax */
  int32_t profile;  /* != 0: record HIP events around the SpMV launches (see zzz_profile_get) */
  int32_t single_reduction; /* != 0: PETSc's -ksp_cg_single_reduction (KSPCGUseSingleReduction): the same CG
                             * with the recurrences s = A z, w = s + b w, <p,w> by recurrence, so that one
                             * iteration needs ONE fused reduction of (<r,z>, <z,s>, norm) instead of two.
                             * ZZZ_CG_PETSC + ZZZ_OP_CSR only. */
  int32_t error_if_not_converged; /* PETSc's -ksp_error_if_not_converged: != 0 makes a solve that ends with a negative
                                   * KSPConvergedReason (DTOL, NaN/Inf, max_it) fail with ZZZ_ERR_DIVERGED.  0 (the
                                   * default, as in PETSc): the solve returns ZZZ_OK with its iteration count, like
                                   * solver.solve() in solver_function (src/poisson_problem.cpp:172-178), and the
                                   * reason is read from zzz_cg_info */
  double rtol;      /* -ksp_rtol / rtol */
  double atol;      /* -ksp_atol (PETSc default 1e-50); unused by ZZZ_CG_CGH */
  double dtol;      /* -ksp_divtol: KSPConvergedDefault stops with KSP_DIVERGED_DTOL once the norm reaches
                     * dtol x the initial norm (zzz_cg_info then reports reason -4, as KSPGetConvergedReason would);
                     * <= 0 selects PETSc's default 1e4 (KSPCreate sets
                     * divtol = 1.e4); unused by ZZZ_CG_CGH (src/cg.h has no such test) */
  /* (added in round 3 behind the fields above, whose layout is unchanged) */
  int32_t pc_degree; /* ZZZ_PC_CHEBYSHEV_JACOBI: Chebyshev steps per application (0 selects 3) */
  int32_t pc_esteig_its; /* ZZZ_PC_CHEBYSHEV_JACOBI: Jacobi-PCG iterations on a noise vector whose Lanczos coefficients give
                          * the estimate of the largest eigenvalue of D^-1 A (PETSc's -ksp_chebyshev_esteig, safety factor
                          * 1.1); the bound used is min(Gershgorin's, 1.1 x estimate).  0 selects 10, < 0 Gershgorin alone */
  double pc_ratio;   /* ZZZ_PC_CHEBYSHEV_JACOBI: upper / lower bound of the targeted spectrum (<= 1 selects 60; ZZZ_PC_MG: 10) */
  /* (added with ABI version 7 behind the fields above, whose layout is unchanged; zero selects the defaults) */
  int32_t pc_mg_levels;          /* ZZZ_PC_MG: most levels (-pc_mg_levels); 0: as many as the coarse limit asks for, <= 12 */
  int32_t pc_mg_coarse_eq_limit; /* ZZZ_PC_MG: the coarsest level is the first with at most this many scalar dofs; 0 selects
                                  * 1000, what the reference's README.md passes to GAMG (-pc_gamg_coarse_eq_limit 1000) */
} zzz_solver_opts;

/* ---- library / device ------------------------------------------------------------------ */

/* Number of visible GPUs; 0 when there is none (then zzz_ctx_create fails with ZZZ_ERR_NO_GPU). */
int zzz_device_count(void);
/* hipMemGetInfo of a device in bytes (for the driver's --memory_profiling log, src/mem.cpp:18-38). */
int zzz_device_memory(int device, size_t* free_bytes, size_t* total_bytes);

/* Creates a context on `device`.  Replaces MPI_Init/PetscInitialize as far as this path needs
 * them (src/main.cpp:245-258). */
int zzz_ctx_create(int device, zzz_ctx** out);
void zzz_ctx_destroy(zzz_ctx* ctx);

/* Message of the last error on ctx (or of the last context-less error when ctx == NULL).
 * The pointer stays valid until the next call on that context. */
const char* zzz_last_error(const zzz_ctx* ctx);

/* Blocks until all enqueued work is done (the driver calls it before stopping a ZZZ timer). */
int zzz_sync(zzz_ctx* ctx);

/* ---- problem data (feed) --------------------------------------------------------------- */

/* mesh::Geometry::x() and the geometry dofmap of the mesh handed to problem()
 * (src/poisson_problem.h:19-23; created at src/mesh.cpp:184-186).
 * x: nverts*3 row-major; cell_verts: ncells*4 local vertex indices.
 * A successful call FORGETS the dofmap and everything behind it -- the Dirichlet set and its values, the exterior facets,
 * the coefficients, the internal dof and cell orders, pattern, matrix, matrix-free plan and near-nullspace: all of them
 * were indexed by the cells or dofs of the mesh just replaced.  Until the next zzz_dofmap_upload every entry point that
 * needs a dofmap answers ZZZ_ERR_ARG ("... before zzz_dofmap_upload", or the missing pattern / matrix it would have
 * built from one): a host-side test in front of every launch, nothing is enqueued.  A multigrid hierarchy of the old
 * problem is no longer served either (zzz_mg_info, _apply, _transfer, _level_csr: "no hierarchy").  A refused call (a bad array) leaves
 * the context as it was.  zzz_dofmap_upload may be called again on the same mesh (another order or block size): the
 * context is then what a fresh one is after the same mesh and that dofmap -- the Dirichlet set, facets and coefficients
 * are uploaded again after it, as after the first.
 * (No ABI version bump: nothing an entry point reads or writes has changed.) */
int zzz_mesh_upload(zzz_ctx* ctx, int64_t nverts, const double* x, int64_t ncells, const int32_t* cell_verts);

/* fem::create_functionspace's DofMap + IndexMap (src/poisson_problem.cpp:43-44,
 * src/elasticity_problem.cpp:108-111).  order 1..3 (form_*.at(order-1),
 * src/poisson_problem.cpp:117); bs 1 or 3; cell_dofs: ncells*nd block indices, nd = 4/10/20. */
int zzz_dofmap_upload(zzz_ctx* ctx, int order, int bs, const int32_t* cell_dofs, int64_t n_owned, int64_t n_ghost);

/* fem::DirichletBC(u0, bdofs) (src/poisson_problem.cpp:53-77, src/elasticity_problem.cpp:119-145): WHERE u is prescribed.
 * bc_dofs: local SCALAR dof indices, owned and ghost; their value is 0 (the reference's u0) until zzz_bc_values_upload
 * says otherwise, and again after every call of this function. */
int zzz_bc_upload(zzz_ctx* ctx, int64_t nbc, const int32_t* bc_dofs);

/* The values of u0 behind that DirichletBC when u0 is not the zero function: bc->dof_values() / u0->x() of
 * fem::DirichletBC(u0, bdofs) (src/poisson_problem.cpp:53-77, src/elasticity_problem.cpp:119-145), consumed by
 * fem::apply_lifting(b, {a}, {{bc}}, {}, 1.0) and bc->set(b) (src/poisson_problem.cpp:152-155,
 * src/elasticity_problem.cpp:226-229; the action form: src/cgpoisson_problem.cpp:159-168).
 * values: (n_owned + n_ghost) * bs doubles in the caller's local numbering, owned then ghosts, exactly like
 * zzz_coeff_upload: u0 at every dof.  Only the entries at constrained dofs are ever read; whatever the others hold
 * (NaN and Inf included) reaches no result.  NULL clears the values: the context is back to u0 == 0.
 * With values present zzz_assemble_vector produces DOLFINx's vector (scale 1, x0 empty):
 *   owned unconstrained row i:  b_i = L_i - sum_cells sum_{j constrained in the cell} A_e[i][j] g_j,  A_e the
 *                               UNCONSTRAINED element matrix of form a (the entries zzz_assemble_matrix computes before it
 *                               zeroes rows and columns); cells in the row's adjacency order, local columns ascending,
 *                               no atomics: the same bits in every run;
 *   owned constrained row i:    b_i = g_i.
 * Without values (or after NULL) zzz_assemble_vector enqueues exactly the kernels it did before this entry point existed.
 * Owned rows are complete locally (ghost-cell layer) and g at ghost dofs comes from this upload: no communication.
 * Solves: with ZZZ_OP_CSR nothing changes -- constrained rows are identity rows, u[bc] converges to g.  ZZZ_OP_MATFREE
 * zeroes the constrained ROWS of its action (src/cgpoisson_problem.cpp:207), so with values present it iterates on b
 * with the constrained entries taken as zero (what scale 0.0 leaves there, :168; the caller's b is not modified);
 * ZZZ_CG_PETSC then writes u[bc] = g when it ends, ZZZ_CG_CGH leaves u[bc] at the caller's initial guess like src/cg.h.
 * Call order: after zzz_dofmap_upload / zzz_cube_generate AND after a Dirichlet set exists (zzz_bc_upload /
 * zzz_cube_generate); ZZZ_ERR_ARG with the reason otherwise.  Whatever changes the dof layout or the Dirichlet set CLEARS
 * the values: zzz_dofmap_upload, zzz_bc_upload, zzz_cube_generate, zzz_ghost_layer_build -- after the last of these the
 * caller uploads values again, for the sizes zzz_local_sizes then reports (the new ghosts included).
 * The matrix does not depend on u0: an upload leaves a multigrid hierarchy, the Chebyshev bound and the product's forms
 * valid.  Time-dependent values: upload again and call zzz_assemble_vector again.  One Dirichlet object; apply_lifting's
 * x0 and scale arguments are not served. */
int zzz_bc_values_upload(zzz_ctx* ctx, const double* values);

/* Exterior facets integrated by the `ds` term of L (src/Poisson.py:32); what
 * create_entities(2)/create_connectivity(2,3) prepare (src/main.cpp:147-148).
 * pairs: nfacets*(cell, local facet 0..3); local facet f is opposite local vertex f. */
int zzz_facets_upload(zzz_ctx* ctx, int64_t nfacets, const int32_t* cell_facet_pairs);

/* Nodal values of a coefficient Function (f->interpolate / g->interpolate,
 * src/poisson_problem.cpp:83-106, src/elasticity_problem.cpp:153-176): (n_owned+n_ghost)*bs. */
int zzz_coeff_upload(zzz_ctx* ctx, int which, const double* values);

/* The whole feed above for the reference's structured cube problems, generated on the device in
 * closed form instead of uploaded: create_cube_mesh's box of nx*ny*nz sub-cubes x 6 tetrahedra
 * (src/mesh.cpp:184-186) cut into `nparts` z-slabs, the P_order function space, the Dirichlet set and
 * the interpolated coefficients of problem() (src/poisson_problem.cpp:33-106,
 * src/elasticity_problem.cpp:101-176) and the halo plan.  Equivalent to uploading the arrays of
 * zzzh_part_create() (include/zzz_host.h); problem = ZZZ_FORM_POISSON | ZZZ_FORM_ELASTICITY.
 * info (optional, 6 entries): global scalar dofs, global cells, owned block dofs, ghost block dofs,
 * global block index of local dof 0, local cells. */
int zzz_cube_generate(zzz_ctx* ctx, int problem, int order, int64_t nx, int64_t ny, int64_t nz, int nparts, int part,
                      int64_t* info);

/* ---- matrix ---------------------------------------------------------------------------- */

/* fem::petsc::create_matrix(*a) (src/poisson_problem.cpp:122-123): sparsity pattern of the
 * owned rows + the dof->cell adjacency the assembly kernels walk.  Outside `ZZZ Assemble
 * matrix`, inside `ZZZ Assemble`, as in the reference. */
int zzz_csr_pattern_build(zzz_ctx* ctx);

/* Sizes of the local matrix: owned scalar rows, local scalar columns (owned+ghost), nonzeros. */
int zzz_csr_sizes(const zzz_ctx* ctx, int64_t* nrows, int64_t* ncols, int64_t* nnz);

/* Copies the CSR arrays to the host (parity checks; MatView-like).  NULL pointers are skipped.
 * rowptr: nrows+1, cols/vals: nnz. */
int zzz_csr_download(zzz_ctx* ctx, int32_t* rowptr, int32_t* cols, double* vals);
/* The row pointers in 64 bits (PetscInt of the reference's CI build): the only form for matrices of 2^31 nonzeros
 * or more (Poisson P3 at 50 M dofs: 2.4 G), where zzz_csr_download(rowptr != NULL) fails with ZZZ_ERR_LIMIT. */
int zzz_csr_rowptr64_download(zzz_ctx* ctx, int64_t* rowptr);

/* Replaces the matrix values (testing the solver on a given operator). vals: nnz. */
int zzz_csr_upload_values(zzz_ctx* ctx, const double* vals);

/* The `ZZZ Assemble matrix` block (src/poisson_problem.cpp:125-139,
 * src/elasticity_problem.cpp:199-213): tabulate_tensor of form a per cell, constrained rows and
 * columns zeroed, ADD into A, then set_diagonal = 1.0 on constrained rows. */
int zzz_assemble_matrix(zzz_ctx* ctx, int form);

/* The `ZZZ Assemble vector` block (src/poisson_problem.cpp:146-157,
 * src/elasticity_problem.cpp:220-231): cell (+ exterior-facet) integrals of L into b,
 * apply_lifting (identically zero while u0 == 0; a pass of its own over the rows next to the Dirichlet set once
 * zzz_bc_values_upload has given u0 values), bc->set. */
int zzz_assemble_vector(zzz_ctx* ctx, int form);

/* ---- vectors --------------------------------------------------------------------------- */

/* Host <-> device copies of b or u; n_owned*bs entries (owned part). */
int zzz_vec_download(zzz_ctx* ctx, int which, double* out);
int zzz_vec_upload(zzz_ctx* ctx, int which, const double* in);

/* la::norm(*u->x()) (src/main.cpp:229): l2 norm over owned entries, summed over all ranks. */
int zzz_vec_norm(zzz_ctx* ctx, int which, double* out);

/* y = A x on host vectors of the owned size (ghost values of x are exchanged first when a
 * communicator is attached).  MatMult; for parity checks of the SpMV kernel alone.
 * Non-finite x: the product runs on an operator stream that leaves out the entries whose assembled value is exactly
 * zero (what MAT_IGNORE_ZERO_ENTRIES does to an AIJ matrix [EXT]) and pads aligned slices with +0.0 entries pointing
 * at a neighbouring column of the same slice.  For finite x that changes no bit of y.  For x with Inf/NaN it does:
 * PETSc's MatMult on the full pattern yields NaN in every row that has a STRUCTURAL entry in such a column (0 * NaN);
 * this product yields NaN in every row with a NONZERO entry there, may miss rows whose only coupling to that column
 * is an exact zero, and may add rows of the same 64-row slice through a padding entry.  The CG iterations see a
 * non-finite vector only after they have broken down (reported as KSP_DIVERGED_NANORINF either way).  ZZZ_SELLP_DROP=0
 * with ZZZ_SELLP_FORMS=5 (no aligned slices) keeps every structural entry and no padding on a real column: NaN then propagates exactly
 * as in the serial CSR loop (tested). */
int zzz_spmv(zzz_ctx* ctx, const double* x, double* y);

/* Measurement aid: HIP-event time of `reps` back-to-back launches of the CG SpMV kernel
 * (w = A p with the <p,w> partials) on the context's stream; variant < 0 keeps the configured
 * kernel variant; otherwise a bit set for A/B runs: bit 0 non-temporal loads, bit 1 unused (ignored),
 * bit 3 the operator stream of zzz_sellp.hip when one was built (default 9 = stream + non-temporal),
 * bit 4 int32 instead of packed 16-bit columns in the tile kernel. */
int zzz_spmv_time(zzz_ctx* ctx, int reps, int variant, double* avg_ms);

/* y = action(x): the matrix-free operator lambda of cgpoisson (src/cgpoisson_problem.cpp:193-230):
 * assemble_vector of form M = action(a, un) with un = x, rows of constrained dofs zeroed, ghosts
 * of x updated first.  Needs mesh, dofmap and Dirichlet dofs only: no pattern, no matrix (the reference's cgpoisson
 * creates neither, src/cgpoisson_problem.cpp:47-247).  Builds the operator's plan on first use (zzz_matfree_setup).
 * Block size 3 (a dofmap uploaded or generated for elasticity): y = A x for form a of src/Elasticity.py, inner(sigma(u),
 * eps(v)) dx with E = 1e6, nu = 0.3, applied cell by cell and never stored; x and y hold 3 n_owned doubles, the three
 * components of a node side by side, and the rows of constrained SCALAR dofs are exactly 0 (a Dirichlet set may constrain
 * one component of a node).  zzz_matfree_setup, _info, _diagonal and zzz_action_time serve both block sizes; a mesh whose
 * smallest cell block touches more nodes than LDS holds is refused with ZZZ_ERR_LIMIT and the context stays usable (the
 * two-pass fallback exists for block size 1 only); zzz_cg_solve(op = ZZZ_OP_MATFREE) returns the same refusal before it
 * writes u or any other vector of the solve.  The float entry points keep declining block size 3.
 * Non-finite input (zzz_action and zzz_action_f32 alike): an Inf or NaN in x[d] stays with the cells that hold d.  y[d] is
 * non-finite (d unconstrained); rows of constrained dofs are 0 whatever their cells carry; the entries of the other dofs
 * that share a cell with d are non-finite wherever the element arithmetic couples them to d -- all of them for P1, for
 * P2/P3 all but those the factorised tables' exact zeros keep apart -- and every dof that shares no cell with d keeps the
 * bits of the clean action.  Nothing lingers: the next action of a finite x gives the clean bits. */
int zzz_action(zzz_ctx* ctx, const double* x, double* y);

/* What cgpoisson sets up once before its solve: fem::create_form of M (src/cgpoisson_problem.cpp:133-145), the
 * coefficient storage of `un` (:182) and the Scatterer with its buffers (:187-190).  Here: the plan of the one-pass
 * matrix-free kernel (csrc/zzz_matfree.hip) -- cells cut into blocks by the Morton order of their centroids, block-local
 * dof lists and 16-bit indices, the order in which a block adds its element vectors, P2/P3 geometry factors.  Optional:
 * zzz_action and zzz_cg_solve(op = ZZZ_OP_MATFREE) build it on first use.  Invalidated by mesh, dofmap and bc uploads. */
int zzz_matfree_setup(zzz_ctx* ctx);
/* info[0] plan valid, [1] cell blocks, [2] cells per block, [3] threads per workgroup, [4] most dofs a block touches,
 * [5] dofs shared between blocks, [6] their partial sums per action, [7] bytes one action addresses (plan + vectors). */
int zzz_matfree_info(zzz_ctx* ctx, int64_t info[8]);
/* diag[n_owned * block size] = the diagonal of the operator zzz_action applies, as the assembled matrix holds it (MatGetDiagonal after
 * fem::set_diagonal: 1.0 on constrained rows, src/poisson_problem.cpp:146-157) -- computed from the element matrices in
 * the matrix-free kernel's pass, nothing assembled.  It is what PCJACOBI uses when zzz_cg_solve runs KSPCG on
 * op = ZZZ_OP_MATFREE (an extension: the reference's KSP path always multiplies with the assembled AIJ matrix,
 * src/poisson_problem.cpp:159-181; same mathematics, the operator recomputed per product instead of streamed). */
int zzz_matfree_diagonal(zzz_ctx* ctx, double* diag);
/* The `ZZZ Assemble vector` block of the matrix-free problem types (src/cgpoisson_problem.cpp:147-170 and its elasticity
 * twin) WITHOUT a sparsity pattern: fills b as zzz_assemble_vector does -- same forms, coefficients, Dirichlet set, lifting
 * once zzz_bc_values_upload has given values, the same ZZZ_ERR_ARG for an unknown form or a missing coefficient -- on the
 * cell-block plan of zzz_matfree_setup (built on first use) instead of the dof -> cell adjacency of the pattern build.
 * Needs mesh, dofmap, Dirichlet dofs, coefficients and, for Poisson, the facets; never calls or needs zzz_csr_pattern_build
 * and creates no pattern (zzz_csr_sizes keeps answering "no sparsity pattern yet").  b is in the caller's numbering, owned
 * rows are complete without communication (u0 at ghost dofs comes from the upload); rows of constrained scalar dofs are
 * exactly 0.0, or u0 with values.  Entries of the uploaded values off the Dirichlet set reach no result.  Every call, and a
 * rebuilt plan, gives the same bits; they are not zzz_assemble_vector's bits (the cells are summed in another order), the
 * two agree to rounding and coexist on one context in either order.  Where the plan cannot be built (the refusal described
 * at zzz_action, either block size) the call returns ZZZ_ERR_LIMIT naming zzz_csr_pattern_build + zzz_assemble_vector as
 * the way out, writes nothing and leaves the context usable.  (A new entry point: ZZZ_ABI_VERSION is unchanged.) */
int zzz_matfree_assemble_vector(zzz_ctx* ctx, int form);
/* Measurement aid, as zzz_spmv_time: HIP-event time of `reps` back-to-back actions w = action(p) with the <p,w>
 * partials (what one iteration of linalg::cg launches at src/cg.h:62,65). */
int zzz_action_time(zzz_ctx* ctx, int reps, double* avg_ms);

/* ---- single precision: the cgpoisson path with T = float ----------------------------------
 * src/cgpoisson_problem.cpp:28 says `using T = PetscScalar` and src/cg.h:18-86 is `template <typename U>`: on a
 * single-precision PETSc the reference runs the action, the halo and linalg::cg in float.  These entry points are that
 * instantiation on one rank, beside the double path, which they leave untouched: the operator's plan is shared, only its
 * value arrays (geometry factors, reference tables, P1 coordinates, partial sums) get float twins, built by the first
 * float action and dropped with the plan.  G = |detJ| K K^T is computed in double and rounded; P1 coordinates are stored
 * relative to an origin of their cell block (subtracted in double): a rounded coordinate is then off by 2^-25 of its distance
 * from that origin, not from the domain's.  The origin is checked against every cell of the block: the float Jacobian is
 * compared with the double one entry by entry, against the cell's extent along that axis, and the float determinant must be
 * safely non-zero.  The block's first listed dof stays the origin within 2^-16; past it the better of it and a second origin
 * -- where the block's cells are finest -- is taken; and where neither keeps the Jacobian within 2^-12 the float action is
 * REFUSED: ZZZ_ERR_LIMIT with a message that names the blocks and the worst distance / extent (a mesh graded towards both
 * ends of a block by 10^5 and more).  A refusal builds no float twin and leaves the plan, the vectors and the double path as
 * they were; zzz_cg_solve_f32 refuses before it touches u.  A float action never returns ZZZ_OK with entries that a cell's
 * collapsed determinant made non-finite.  Declined with ZZZ_ERR_ARG and a reason: block size 3, an attached communicator. */

/* y = action(x) in float (src/cgpoisson_problem.cpp:193-230 with T = float): host arrays of n_owned floats, as zzz_action
 * takes doubles.  Bit-reproducible from call to call. */
int zzz_action_f32(zzz_ctx* ctx, const float* x, float* y);
/* Measurement aid, as zzz_action_time: `reps` float actions with the <p,y> partials (src/cg.h:62,65 with U = float). */
int zzz_action_time_f32(zzz_ctx* ctx, int reps, double* avg_ms);
/* info[0] the float twins are built, [1] bytes one float action addresses (zzz_matfree_info's [7] in double), [2] bytes of
 * LDS a workgroup of the float action uses for its block (src/cgpoisson_problem.cpp:182, the storage of `un`, in float),
 * [3] workgroups per CU that leaves room for. */
int zzz_matfree_info_f32(zzz_ctx* ctx, int64_t info[4]);

/* `ZZZ Create near-nullspace`: build_near_nullspace of src/elasticity_problem.cpp:36-94 (called at :233-244) -- the six
 * rigid-body modes of the vector-valued space at the dof coordinates (tabulate_dof_coordinates: every dof's reference
 * node pushed through its cell's affine map), orthonormalised in basis order as la::orthonormalize does, checked as
 * la::is_orthonormal does (error "Space not orthonormal" otherwise; *max_deviation = largest |<x_i,x_j> - delta_ij|).
 * Inner products over the owned entries, summed over the ranks (collective with a communicator attached).  The
 * rotations are taken about the centre of the dofs: the same basis in exact arithmetic, and no digits lost to the
 * projection on a mesh far from the origin.  The
 * reference passes the basis to MatSetNearNullSpace for GAMG; Jacobi-CG does not consume it. */
int zzz_near_nullspace_build(zzz_ctx* ctx, double* max_deviation);
/* mode k (0..5) of that basis, owned part, 3 * n_owned entries in the caller's numbering */
int zzz_near_nullspace_download(zzz_ctx* ctx, int k, double* out);

/* ---- the reference's native partition ----------------------------------------------------- */

/* Global indices of the local block dofs (index_map.local_to_global: owned, then ghosts) and of the local mesh
 * vertices: what two ranks use to recognise a shared dof or vertex.  Needed by zzz_ghost_layer_build only. */
int zzz_global_ids_upload(zzz_ctx* ctx, const int64_t* dof_global, const int64_t* vert_global);
/* ... of the local block dofs as they are now (after zzz_ghost_layer_build: with the new ghosts) */
int zzz_global_ids_download(zzz_ctx* ctx, int64_t* dof_global);

/* Collective.  For a feed partitioned as the reference partitions it -- mesh::create_cell_partitioner(
 * GhostMode::none), src/mesh.cpp:182-183: every rank holds its own cells only, so the matrix rows and vector
 * entries of dofs on the partition interface are incomplete locally and the reference completes them in every
 * assembly by MatAssemblyBegin/End (src/poisson_problem.cpp:132-133) and b.scatter_rev(std::plus) (:154).
 * Call after mesh, dofmap, Dirichlet dofs, exterior facets, coefficients, the forward-scatter plan
 * (zzz_halo_upload) and the global indices have been uploaded: the ranks exchange ONCE the cells that touch a
 * neighbour's dofs, every rank appends what it receives as ghost cells (new ghost dofs join the forward scatter
 * of their owners) and from then on assembles complete owned rows with no exchange per assembly: A and b equal
 * the reference's after its MatAssembly / scatter_rev.  zzz_local_sizes reports the extended sizes. */
int zzz_ghost_layer_build(zzz_ctx* ctx);
/* sizes = {vertices, cells, owned block dofs, ghost block dofs, cells the caller uploaded, neighbours} */
int zzz_local_sizes(const zzz_ctx* ctx, int64_t sizes[6]);

/* The library keeps the owned dofs in an INTERNAL locality order of its own (computed from geometry when the dofmap
 * is uploaded: lexicographic by lattice cell, entity type by entity type -- csrc/zzz_renumber.hip), so that its speed does
 * not depend on the numbering DOLFINx's partitioner and reordering happened to produce (src/mesh.cpp:153-162,182-186).
 * Every index and vector of this ABI is in the CALLER's numbering; the translation is the library's business.  Two
 * things are visible all the same: (1) MatMult sums a row in ascending INTERNAL column order, so zzz_spmv (and the CG
 * iterates) equal the serial CSR loop bit for bit on the internally ordered system P A P^T, and the caller-ordered loop
 * only to round-off -- exactly as PETSc's result depends on the local numbering of the run; (2) this function, which
 * returns P: perm[i] = caller index of internal owned block dof i (the identity when the caller's order was kept:
 * structured feeds of this repository, meshes that are not a lattice, ZZZ_RENUMBER=0).  kind (optional): low bits 0 caller's
 * dof order kept, 1 lattice order, 2 coordinate-bin order (ZZZ_RENUMBER=2 only); bit 4 (16): the CELLS are kept in an
 * internal order as well (simplex type by simplex type, lattice cube by lattice cube) -- invisible at this ABI except
 * that an entry of A or b is then the sum of its cells' contributions in that order instead of the caller's cell
 * order (the same terms; differences of the last bits).  No reference counterpart. */
int zzz_internal_order_download(zzz_ctx* ctx, int32_t* perm /* n_owned */, int32_t* kind);

/* ---- solve ----------------------------------------------------------------------------- */

/* solver_function(u, b) (src/poisson_problem.cpp:164-179; src/cgpoisson_problem.cpp:178-244;
 * called under `ZZZ Solve` at src/main.cpp:208-211).  Solves A u = b with the vectors held by
 * the context; returns the Krylov iteration count like KSPGetIterationNumber / cg()'s k.
 * rnorm[0] = final norm, rnorm[1] = initial norm (variant CGH: <r,r> and <r0,r0>).  With a communicator the solve is
 * collective; that holds for pc = ZZZ_PC_MG on several ranks too (set-up, every cycle's halo exchanges and its all-reduce
 * of the level-1 right-hand side, the all-reduced scalars: all ranks stop together). */
int zzz_cg_solve(zzz_ctx* ctx, const zzz_solver_opts* opts, int* iters, double* rnorm);
/* linalg::cg<float> (src/cg.h:38-86 with U = float, called at src/cgpoisson_problem.cpp:233) on the float action: x, r,
 * p, y are float device vectors, alpha and beta floats as `const U alpha`, `const U beta` are (:65,75).  DIFFERENCE: the
 * sums behind <p,y> and <r,r> are accumulated in double and rounded once, where the reference accumulates them in U --
 * more accurate, and deterministic.  b is read from the context's double b, x starts from its u (the initial guess, :39)
 * and the solution is stored there as doubles: zzz_vec_download, zzz_vec_norm, zzz_cg_history and zzz_cg_info serve both
 * precisions.  rnorm as for ZZZ_CG_CGH.  Accepted: variant ZZZ_CG_CGH, pc ZZZ_PC_NONE, op ZZZ_OP_MATFREE.  Declined with
 * ZZZ_ERR_ARG and the reason, the context staying usable: any other variant, preconditioner or operator,
 * single_reduction, block size 3, an attached communicator, Dirichlet values uploaded by zzz_bc_values_upload. */
int zzz_cg_solve_f32(zzz_ctx* ctx, const zzz_solver_opts* opts, int* iters, double* rnorm);

/* Residual-norm history of the last solve (KSPGetResidualHistory): copies min(n, iters+1). */
int zzz_cg_history(zzz_ctx* ctx, int n, double* out);

/* About the last zzz_cg_solve: info[0] bit 0 is reserved and always 0; bit 1 (value 2)
 * when Jacobi's inverse diagonal was read as 16-bit codes into a table of its distinct values and z = D^-1 r recomputed
 * instead of stored (68 instead of 80 B per row and iteration in the two vector kernels; the same bits), bits 8-31 = those
 * distinct values, bit 32 set when there were at most 256 of them and the codes were 8 bits wide (66 B); bit 2 (value 4) when the solve was ZZZ_CG_PIPE with a communicator and its all-reduces ran on a stream of
 * their own beside the halo exchange and the product (not with the host-mediated local backend, nor with mailboxes
 * between contexts of one process);
 * info[1] = its iteration count (same iterates, bit for bit, either way); info[2] = how it ended, in
 * KSPConvergedReason's numbering: 2 KSP_CONVERGED_RTOL, 3 KSP_CONVERGED_ATOL, -3 KSP_DIVERGED_ITS (max_it / kmax
 * reached), -4 KSP_DIVERGED_DTOL, -9 KSP_DIVERGED_NANORINF; info[3] = with ZZZ_PC_CHEBYSHEV_JACOBI the upper bound of
 * the spectrum of D^-1 A the polynomial was built on, x 1e6 (0 otherwise). */
int zzz_cg_info(zzz_ctx* ctx, int64_t info[4]);

/* Average duration (ms) and count of the SpMV launches event-timed during the last
 * zzz_cg_solve with opts.profile != 0. */
int zzz_profile_get(zzz_ctx* ctx, double* spmv_avg_ms, int64_t* spmv_count);

/* Storage the CG SpMV streams for the current matrix (no reference counterpart: MatMult on AIJ reads
 * 12 B per nonzero, src/poisson_problem.cpp:168-177 [EXT]).  info[0] = 1 when the column stream is the
 * 16-bit band code (10 B per nonzero), 0 for int32 columns; info[1] = offset bits of the code;
 * info[2] = tiles left on int32 columns; info[3] = number of tiles; info[4] = lanes per row of the row sums
 * (1: a row's products are added in column order like the scalar CPU loop; L > 1, chosen for rows of
 * >= 128 nonzeros on average: lane j adds the j-th contiguous chunk of ceil(len/L) products in column
 * order, chunk sums combined pairwise ((c0+c1)+(c2+c3))+...); info[5] = 1 when the SpMV runs on the sliced-ELL
 * copy (chosen for matrices small enough to stay cache-resident between CG iterations; same column-order row
 * sums, bit-identical results) instead of the CSR tile kernel; info[6..7] = 0. * When the stream carries x windows (block size 3: the columns a group of 256 rows reaches are loaded into LDS once per
 * group, the stream's codes are window indices) info[3] = -(LDS doubles per workgroup) and info[2] = bytes of x those
 * loads move per product. */
int zzz_spmv_info(zzz_ctx* ctx, int64_t info[8]);
/* The values of the operator stream (csrc/zzz_sellp.hip): info[0] = 0 when the product reads them as doubles, 1 / 2 when it
 * reads 16-bit codes into a dictionary of the matrix's DISTINCT values held in memory / copied into LDS by every workgroup
 * (matrices of regular meshes hold few: ~1 300 at 10 M-dof P1 Poisson; at most 65 535 qualify; same doubles, same
 * order of operations, bit-identical products); info[1] = distinct values (+0.0 included); info[2] = bytes per product of
 * the stream in the form in use; info[3] = bytes per product with the values as doubles; info[4] = 1 when the stream is
 * one of one-chunk slices and the product runs on the kernel for those (csrc/zzz_sellp_pipe.hip: two rows per lane), else 0;
 * info[5] = workgroups per CU of the product's persistent grid.  0s when the product does not run on the stream.
 * zzz_spmv_values_info writes info[0..3] only (its signature of round 4: a caller built against that header passes four
 * entries); everything from info[4] on comes through zzz_spmv_values_info2, which writes the first min(n, 14) entries:
 * info[6] = 1 when the product of a block-size-3 matrix runs in block-row form (csrc/zzz_sellp_blk.hip: one lane per node,
 * 16-bit codes into a table of the matrix's distinct 3 x 3 blocks in LDS), info[7] = entries of that table (zero block
 * included), info[8] = chunks of 16 block slots per node, info[9] = 1 when the table's rows (nine doubles each) sit in LDS, 2 when
 * they are rows of nine 16-bit value offsets in memory and the VALUES sit in LDS (more than 2 200 distinct blocks; then
 * info[7] still counts the blocks); info[2] is then the bytes of THAT form.  Where info[4] = 1: info[10] = slices whose value
 * codes the kernel reads PACKED (4-bit indices into per-slot palettes of 16 codes: 512 B per slice for 1 024; ZZZ_SELLP_PAL=0:
 * none), info[11] = slices read as 16-bit codes, info[12] = pairs of slices of one of either, info[13] = the most distinct
 * codes met in one slot of one slice (a slice is packed when no slot holds more than 16). */
int zzz_spmv_values_info(zzz_ctx* ctx, int64_t info[4]);
int zzz_spmv_values_info2(zzz_ctx* ctx, int n, int64_t* info);
/* The path the last zzz_csr_pattern_build took through its kernels and fallbacks (csrc/zzz_pattern.hip), for
 * tests that pin a connectivity to a path: info[0] = how the dof -> cell adjacency was built: 1 without a sort, from the
 * monotone runs of the connectivity, 2 by the radix sort from the start, 3 by the sort after a window of the sort-free build
 * overflowed (the next build of the same dofmap answers 2: it remembers), 0 on the host; info[1] = the runs it was built
 * from (0 unless info[0] = 1); info[2] = P1: 16 or 32, the column cap of the thread-per-row kernel that sufficed, 0 when a
 * wavefront per row built the rows (always at P2 / P3), -1 on the host; info[3] = the builder: 0 device, 1 host after the
 * device refused (a row of more candidate columns than it holds), 2 host by ZZZ_PATTERN=host; info[4] = unique block columns
 * of the longest block row; info[5] = 1 when the transposed adjacency came from the P1 pattern kernel, 0 from its own pass;
 * info[6] = 1 when the build left the positions of the element-matrix entries for the P2 / P3 assembly (else it searches the
 * columns); info[7] = 0.  ZZZ_ERR_ARG without a pattern.  (A new entry point: ZZZ_ABI_VERSION is unchanged.) */
int zzz_pattern_info(zzz_ctx* ctx, int64_t info[8]);
/* ---- geometric multigrid (ZZZ_PC_MG, ZZZ_PC_PMG) ----------------------------------------------
 * PCSetUp(PCMG) behind solver.set_from_options() (src/poisson_problem.cpp:169; README.md:59-146): builds the hierarchy
 * for these options, or refreshes its values after an assembly.  Optional: zzz_cg_solve(pc = ZZZ_PC_MG) does it on first
 * use, inside the solve, where PETSc's PCSetUp runs.  Overwrites the context's Krylov work vectors (not b, not u).
 * opts->pc == ZZZ_PC_PMG builds the p-multigrid hierarchy, ZZZ_PC_AGG / ZZZ_PC_SAGG / ZZZ_PC_SAGG_RBM the (smoothed) aggregation hierarchy
 * (zzz_mg_info then reports nx = ny = nz = 0 for every level); any other value is read as ZZZ_PC_MG.  One context holds one hierarchy: a set-up
 * of another kind replaces it.  ZZZ_PC_MG on several ranks (see ZZZ_PC_MG): COLLECTIVE; every rank returns the ranks' common
 * status (a rank whose own set-up succeeded while another's failed gets ZZZ_ERR_RCCL and keeps no hierarchy). */
int zzz_mg_setup(zzz_ctx* ctx, const zzz_solver_opts* opts);
/* PCView of that hierarchy.  level < 0: out = {levels, scalar dofs of the coarsest, set-ups done so far (builds and
 * refreshes), products per V-cycle on level 0, device bytes of the coarse levels, HIP-event ms per V-cycle in the last solve
 * with opts.profile != 0 (else 0), host ms of the last set-up that did work (it ends synchronised), levels of order > 1
 * (ZZZ_PC_PMG at order 2 or 3: 1, they come first; else 0)}.  Otherwise that level's
 * {nx, ny, nz, scalar dofs, nonzeros, hi, lo, smoother degree} (hi = lo = degree = 0 on the coarsest: a dense solve).
 * ZZZ_PC_MG on several ranks: level 0 reports the cells, dofs and nonzeros of the GLOBAL cube (the ranks' owned rows together),
 * so the level table is the same on every rank, and the one-rank run's. */
int zzz_mg_info(zzz_ctx* ctx, int level, double out[8]);
/* PCApply: z = M r, one V-cycle on host vectors of the owned size -- zzz_spmv's counterpart, for parity checks.  ZZZ_PC_MG on
 * several ranks: COLLECTIVE; takes and returns this rank's owned-length vectors. */
int zzz_mg_apply(zzz_ctx* ctx, const double* r, double* z);
/* The grid transfer between level and level + 1 alone (MatInterpolate / MatRestrict of PCMG): dir 0 gives
 * out = P~ in (in: level + 1, out: level), dir 1 gives out = P~^T in.  P~ = F_f P F_c with F zeroing the constrained
 * dofs.  The restriction sums in a fixed order: two calls give the same bits.  ZZZ_PC_MG on several ranks: level 0 moves between
 * this rank's OWNED fine vector and the WHOLE level-1 vector and is COLLECTIVE in both directions (the restriction's result is
 * the ranks' sum, the same on every rank); the levels below are every rank's own. */
int zzz_mg_transfer(zzz_ctx* ctx, int level, int dir, const double* in, double* out);
/* The matrix of a coarse level (1 <= level < levels) as the hierarchy holds it, for parity checks: 64-bit row pointers
 * (scalar dofs + 1), columns and values (zzz_mg_info(level) gives the sizes); any of the three may be NULL. */
int zzz_mg_level_csr(zzz_ctx* ctx, int level, int64_t* rowptr, int32_t* cols, double* vals);
/* The stored prolongator between level and level + 1 of a ZZZ_PC_SAGG or ZZZ_PC_SAGG_RBM hierarchy: 64-bit row pointers (fine scalar dofs + 1),
 * coarse columns, values, fine rows in the caller's numbering on level 0; any of the three may be NULL; out_nnz optional.
 * ZZZ_ERR_ARG for another kind of hierarchy.  (A new entry point: ZZZ_ABI_VERSION is unchanged.) */
int zzz_mg_level_p(zzz_ctx* ctx, int level, int64_t* rowptr, int32_t* cols, double* vals, int64_t* out_nnz);
/* The near-nullspace B that level's orthogonalisation read in a ZZZ_PC_SAGG_RBM hierarchy (the coarsest level: the B_c the
 * level above it wrote), out[6][scalar dofs of the level]: level 0 in the caller's numbering with the entries of constrained
 * dofs 0.  ZZZ_ERR_ARG for another kind of hierarchy.  zzz_mg_info(level) of such a hierarchy reports, in ny's slot (nx = nz = 0:
 * there is no cube), how many of that level's dofs are dropped coarse dofs.  (A new entry point: ZZZ_ABI_VERSION is unchanged.) */
int zzz_mg_level_nns(zzz_ctx* ctx, int level, double* out);
/* How the next ZZZ_PC_SAGG / ZZZ_PC_SAGG_RBM hierarchy of this context forms P, T = A P and A_c = P^T T (csrc/zzz_sagg_rows.hip).
 * ZZZ_MG_PRODUCTS_LISTS (the default): every term written out with a 64-bit key, sorted, the sorted lists kept for the refresh;
 * a level with more terms than 32-bit positions take is declined with ZZZ_ERR_LIMIT.  ZZZ_MG_PRODUCTS_ROWS: row by row -- the
 * patterns from sorted and uniqued (row, column) candidates of a bounded chunk of rows at a time, the values with one
 * accumulator per entry and the summation index ascending -- the SAME sums in the same order, so the same P, R, T, A_c, coarse
 * near-nullspace and drops bit for bit, with no term list kept and no limit on the terms; a level whose A, T or A_c has 2^31
 * or more entries is declined with ZZZ_ERR_LIMIT.  (ZZZ_SAGG_ROWS_BUDGET lowers the candidates per chunk and ZZZ_SAGG_ROWS_LDS the
 * row length, 1024, up to which a row's accumulators sit in LDS: both for tests; ZZZ_SAGG_MAX_TERMS is not read in this mode.)  The mode belongs to the context and survives every upload; it is part of what a smoothed
 * hierarchy was built from: the next set-up or solve after a change rebuilds, a hierarchy built in the current mode is kept
 * and refreshed.  ZZZ_PC_MG, ZZZ_PC_PMG and ZZZ_PC_AGG never read it.  Any other mode: ZZZ_ERR_ARG, nothing changed.
 * (A new entry point: ZZZ_ABI_VERSION is unchanged.) */
enum zzz_mg_products_mode
{
  ZZZ_MG_PRODUCTS_LISTS = 0,
  ZZZ_MG_PRODUCTS_ROWS = 1
};
int zzz_mg_products(zzz_ctx* ctx, int mode);
/* The products of the standing ZZZ_PC_SAGG / ZZZ_PC_SAGG_RBM hierarchy: info[0] = the mode it was built in; info[1] = device
 * bytes its levels keep for P, R, T and the term lists (lists) or the level-0 entry permutation (rows), the coarse matrices
 * excluded; then, of the last build in the rows mode (0 in the lists mode): info[2] = chunks of the symbolic passes, summed
 * over levels and products; info[3] = the most candidates one row had; info[4] = the budget, candidates per chunk;
 * info[5] = rows that formed a chunk alone because they exceeded it; info[6] = the peak of the transient device bytes of the
 * products' set-up; info[7] = 0.  ZZZ_ERR_ARG without a hierarchy or for another kind.  (A new entry point: ZZZ_ABI_VERSION
 * is unchanged.) */
int zzz_mg_products_info(zzz_ctx* ctx, int64_t info[8]);

/* Version of this header's ABI: bumped whenever an existing entry point changes what it reads or writes (7: zzz_cg_solve
 * reads the two pc_mg_* fields behind pc_ratio).  ZZZ_PC_PMG did not bump it: a new enumerator changes no struct, no
 * entry point and nothing that a caller built against the earlier header passes or receives -- such a caller never
 * sends the value 4, and a library without it answers that value with ZZZ_ERR_ARG.  Nor did zzz_bc_values_upload: a new
 * entry point, no struct and no existing entry changed.  ZZZ_PC_AGG (5) and zzz_mg_level_csr: the same two arguments;
 * ZZZ_PC_SAGG (6) and zzz_mg_level_p: the same two again; ZZZ_PC_SAGG_RBM (7) and zzz_mg_level_nns: and again.  zzz_mg_products and zzz_mg_products_info: new
 * entry points, version unchanged. */
#define ZZZ_ABI_VERSION 7
int zzz_abi_version(void);

/* ---- multi-GPU (one context per GPU; RCCL over xGMI) --------------------------------------- */

#define ZZZ_UNIQUE_ID_BYTES 128

/* dlopen librccl.so.1 now (it is otherwise loaded by the first zzz_comm_* call).  For processes that also
 * hold another copy of RCCL -- a Python process that imports torch, which bundles its own -- so that every
 * rank binds the SAME library: call it on every rank before that other copy is loaded.  No reference
 * counterpart (MPI_Init, src/main.cpp:42 [EXT], is the closest). */
int zzz_comm_load(void);
/* File the bound librccl was loaded from (dladdr), "" before zzz_comm_load.  Every rank of a job must report the
 * same library: bench.py compares them before the first collective and exits non-zero on a mismatch. */
const char* zzz_comm_library_path(void);
/* What the multi-GPU path of this context does, for diagnostics (bench.py prints it per rank): info = {ranks,
 * rank, neighbours, bytes sent per forward scatter, bytes received, 1 = halo on its own communicator + stream
 * (ncclCommSplit) / 2 = halo through peer memory (zzz_comm_p2p_halo), 1 = CG scalars through the peer-memory mailboxes, 1 = halo overlapped with the interior rows,
 * interior / boundary work items (groups of 256 rows or tiles) of the product, 1 = host-mediated local backend, mean exposed
 * halo wait per product of the last profiled solve in ns (main stream idle between its interior rows and the halo's arrival)}. */
int zzz_comm_info(zzz_ctx* ctx, int64_t info[12]);

/* ncclGetUniqueId on the root; ship the bytes to the other ranks out of band (the driver's
 * threads share memory; bench.py broadcasts them).  Replaces MPI_COMM_WORLD bootstrap. */
int zzz_comm_unique_id(void* id /* ZZZ_UNIQUE_ID_BYTES */);

/* ncclCommInitRank: attaches this context as `rank` of `nranks`. */
int zzz_comm_init(zzz_ctx* ctx, int nranks, int rank, const void* id);

/* Host-mediated communicator for single-process runs: the `nranks` contexts are driven by `nranks`
 * threads of one process (they may share a GPU); collectives meet at a barrier and exchange through
 * host memory.  Functionally identical to the RCCL path, far slower: meant for validating
 * partitioned runs on a single-GPU machine.  Every rank must make the same sequence of calls. */
int zzz_local_group_create(int nranks, void** group);
void zzz_local_group_destroy(void* group);
/* Break the group: every rank waiting in (or later entering) one of its collectives returns ZZZ_ERR_RCCL instead
 * of waiting for a rank that has failed.  The library does this itself when a rank fails INSIDE a collective. */
void zzz_local_group_abort(void* group);
int zzz_comm_init_local(zzz_ctx* ctx, void* group, int rank);

/* Optional: carry the CG's scalar all-reduces (MPI_Allreduce inside la::inner_product /
 * la::squared_norm, src/cg.h:53,65,74) through peer memory over xGMI instead of ncclAllReduce: each
 * rank exports a small device mailbox, every rank attaches all of them (hipIpcOpenMemHandle between
 * processes, peer access between contexts of one process).  Call after zzz_comm_init /
 * zzz_comm_init_local, on every rank: export, exchange the handles out of band in rank order (as the
 * unique id), attach.  Attach runs test rounds and makes the ranks agree; *enabled = 0 means the
 * communicator's own all-reduce stays in use (never an error).  The mailbox sums in rank order on
 * every rank (bit-identical everywhere); RCCL sums in its own order: the same iteration to round-off. */
#define ZZZ_P2P_HANDLE_BYTES 128
/* A communicator with no transport of its own: only the peer-memory all-reduce and halo below work on it.  For
 * replicated runs and for exercising the peer-memory transport between processes. */
int zzz_comm_init_peer_only(zzz_ctx* ctx, int nranks, int rank);
int zzz_comm_p2p_export(zzz_ctx* ctx, void* handle /* ZZZ_P2P_HANDLE_BYTES */);
int zzz_comm_p2p_attach(zzz_ctx* ctx, const void* handles /* nranks x ZZZ_P2P_HANDLE_BYTES */, int* enabled);
int zzz_comm_p2p_disable(zzz_ctx* ctx);
/* back on after zzz_comm_p2p_disable, only if attach had succeeded; every rank must make the same call */
int zzz_comm_p2p_enable(zzz_ctx* ctx, int* enabled);
/* The same allocation carries a halo window (ZZZ_P2P_HALO_MB, default 64): with the mailboxes enabled, the forward
 * scatter of the product's input vector (common::Scatterer::scatter_fwd inside MatMult, src/poisson_problem.cpp:177;
 * src/cgpoisson_problem.cpp:225-229) is then plain device stores into the NEIGHBOUR's window over xGMI plus an arrival
 * tag, and a copy out of the own window on the receiving side -- no ncclSend / ncclRecv, no communicator in the solve
 * loop at all (a peer-only communicator becomes a complete transport).  Plans that do not fit the window (more than 32
 * neighbours, or a message beyond window / 2 / ranks) keep the communicator's send / recv.  on = 0 keeps the halo on
 * the communicator while the all-reduces stay on the mailboxes (A/B; every rank must make the same call);
 * *in_use = 1 when the next exchange goes through the window.
 * COLLECTIVE, all four: with the mailboxes attached, zzz_comm_p2p_attach, zzz_comm_p2p_enable, zzz_comm_p2p_halo and
 * zzz_halo_upload end in one agreement of all ranks on the exchange's transport (both ends of an exchange must use the
 * same one).  Every rank of the communicator must make the same calls the same number of times, in the same order -- as
 * MPI ranks must for MPI_Comm_dup; the agreement goes through the communicator's own all-reduce (blocking, no time-out)
 * and, on a peer-only communicator, through the mailboxes (a rank that waits ten minutes for the others gives up with
 * ZZZ_ERR_RCCL). */
int zzz_comm_p2p_halo(zzz_ctx* ctx, int on, int* in_use);

/* The forward scatter of common::Scatterer / IndexMap (src/cgpoisson_problem.cpp:187-190,
 * 225-229): for neighbour k, this rank sends x[send_idx[send_off[k]..send_off[k+1])] (owned
 * block dofs) and receives recv_cnt[k] block values into the next ghost slots; the ghost block
 * range is ordered by neighbour, then by the sender's send order. */
int zzz_halo_upload(zzz_ctx* ctx, int nneigh, const int32_t* neigh_rank, const int64_t* send_off,
                    const int32_t* send_idx, const int64_t* recv_cnt);

#ifdef __cplusplus
}
#endif
#endif /* ZZZ_ABI_H */
