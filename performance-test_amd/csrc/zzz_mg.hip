// ZZZ_PC_MG: geometric multigrid preconditioner for the P1 cube problems (PCSetUp / PCApply of PETSc's PCMG behind
// solver.set_from_options(), src/poisson_problem.cpp:169; the reference's README.md:59-146 recommends a multigrid
// preconditioner for every configuration).
//
// Level 0 is the caller's context.  Level l+1 is the SAME problem re-discretised on max(2, (n+1)/2) cells per axis -- a
// child context fed by zzz_cube_generate, patterned by zzz_csr_pattern_build and assembled by zzz_assemble_matrix, on
// the caller's stream; its product is launch_spmv in whatever stream form its matrix gets.  The levels are not nested
// when n is odd.  What is here: the grid transfer (closed form, no P stored), the dense coarsest solve, the V-cycle.  The
// smoother is the Chebyshev-Jacobi polynomial of zzz_cg.hip (ChebPlan, cheb_first, cheb_terms: zzz_cg.h) on the level's
// context, product and term as separate launches; the post-smoother starts from x.  Nothing in the cycle synchronises
// with the host, and every kernel of it returns at once when the solve's stop flag is set.
//
// Transfer, for fine vertex (i_x, i_y, i_z) and axis a (nf / nc: fine / coarse cells of that axis):
//   c_a = min(i_a nc_a / nf_a, nc_a - 1) in 64-bit integers;  f_a = double(i_a nc_a - c_a nf_a) / double(nf_a);
//   axes sorted by descending f, ties to the lower axis: (a1, a2, a3);
//   weights 1 - f_a1, f_a1 - f_a2, f_a2 - f_a3, f_a3 on the coarse vertices c, c + e_a1, c + e_a1 + e_a2, c + e_a1 + e_a2 + e_a3
// -- the Kuhn simplex of the coarse cube that holds the fine vertex (host/cube_layout.h cuts every cube along the same
// diagonal), i.e. the coarse P1 function evaluated there: exact for linear functions, the nested interpolation when
// nf = 2 nc.  c_a and f_a depend on (a, i_a) alone: three small tables per level pair, computed on the host in the
// integers above, so the kernels divide nothing.  P~ = F_f P F_c with F zeroing the constrained dofs.
//
// ZZZ_PC_PMG at order k = 2, 3 puts ONE level in front: level 0 is the caller's Pk matrix, level 1 the same cube at order 1
// (a child context like the others), levels 2.. the hierarchy above of that P1 problem.  The pair (0, 1) is transferred by
// zzz_pmg.hip; smoother, cycle, set-up caching, refresh, stop flag and profiling are the ones here.  At order 1
// ZZZ_PC_PMG is ZZZ_PC_MG.
//
// ZZZ_PC_AGG builds its levels from the matrix instead (zzz_agg.hip: aggregates, P^T A P into child contexts that adopt the
// CSR, the two transfers); everything else -- smoother, cycle, dense solve, caching, refresh, profiling -- is the one here.
// ZZZ_PC_SAGG is ZZZ_PC_AGG with a smoothed prolongator (zzz_sagg.hip), whose damping needs the level's spectrum bound: there
// a level's bound comes before the next level's values, in a build and in a refresh.  ZZZ_PC_SAGG_RBM is ZZZ_PC_SAGG with the
// context's near-nullspace in the tentative prolongator (zzz_sagg_rbm.hip): nodes of 6 dofs on its coarse levels, whose
// contexts are scalar.
//
// ZZZ_PC_MG on several ranks (a communicator of two or more, the cube generated as part `rank` of `nranks` z-slabs): level 0 is
// the caller's slab -- its products exchange the halo, its bound is the ranks' common one (chebyshev_setup) -- and EVERY coarser
// level is whole on every rank, the child contexts of the one-rank hierarchy, built from the global cube's dimensions.  The pair
// (0, 1) moves between the owned fine vector and the whole level-1 vector: the prolongation reads the whole coarse vector, the
// restriction leaves this rank's partial sums and the communicator adds them (comm_allreduce_sum, in its order).  From level 1
// down every rank runs the same cycle on the same numbers, so the preconditioner is the one-rank operator.
//
// The five differ in MgKind alone (a level's transfer, the next level, that level's values); the set-up keeps a
// hierarchy while its MgStructKey holds and the levels' values while its MgValuesKey holds.
#include "zzz_cg.h"
#include "zzz_mg_transfer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

namespace zzz
{
// x_f (+)= P~ e_c: a thread per fine vertex of the window (zzz_mg_transfer.h), four gathers per component, summed in the
// simplex's order
__global__ __launch_bounds__(VB) void k_mg_prolong(const int* __restrict__ stop, MgGeom G, const int32_t* __restrict__ tc,
                                                   const double* __restrict__ tf, const uint8_t* __restrict__ bcf,
                                                   const uint8_t* __restrict__ bcc, const double* __restrict__ ec,
                                                   double* __restrict__ xf, int accumulate)
{
  if (stop && *stop)
    return;
  for (int64_t v = blockIdx.x * (int64_t)VB + threadIdx.x; v < G.nfv; v += (int64_t)gridDim.x * VB)
    mg_prolong_vertex(G, tc, tf, bcf, bcc, ec, xf, accumulate, v);
}

// r_c = P~^T r_f in gather form: a thread per coarse vertex of the planes the window reaches walks the window's fine vertices
// whose simplex can hold it, in ascending (i_z, i_y, i_x) -- no atomics, the same bits in every run.  sub != null:
// r_f = b - sub, the residual formed on the way in (b - A x with sub = A x), which saves the pass that would store it.
template <int BS>
__global__ __launch_bounds__(VB) void k_mg_restrict(const int* __restrict__ stop, MgGeom G, const int32_t* __restrict__ tc,
                                                    const double* __restrict__ tf, const int32_t* __restrict__ rng,
                                                    const uint8_t* __restrict__ bcf, const uint8_t* __restrict__ bcc,
                                                    const double* __restrict__ rf, const double* __restrict__ sub,
                                                    double* __restrict__ rc)
{
  if (stop && *stop)
    return;
  const int64_t c0 = (int64_t)G.cz0 * G.pc[0] * G.pc[1];
  for (int64_t c = blockIdx.x * (int64_t)VB + threadIdx.x; c < G.ncv; c += (int64_t)gridDim.x * VB)
    mg_restrict_vertex<BS>(G, tc, tf, rng, bcf, bcc, rf, sub, rc, c0 + c);
}

// The coarsest level: x = A^-1 b with the dense inverse, a wavefront per row; lane l sums columns l, l + 64, ... in
// ascending order and the 64 sums meet in the shuffle tree -- one fixed order.
__global__ __launch_bounds__(VB) void k_mg_dense(const int* __restrict__ stop, const double* __restrict__ ainv,
                                                 const double* __restrict__ b, double* __restrict__ x, int n)
{
  if (stop && *stop)
    return;
  const int row = blockIdx.x * (VB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n)
    return;
  const double* __restrict__ a = ainv + (size_t)row * n;
  double s = 0.0;
  for (int j = lane; j < n; j += 64)
    s += a[j] * b[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    s += __shfl_down(s, o, 64);
  if (lane == 0)
    x[row] = s;
}

// How a level reaches the next coarser one -- its transfer, and where that level and its matrix values come from: the
// same cube on half the cells (tables above), the same cube at order 1 (zzz_pmg.hip), the aggregates of its matrix
// (zzz_agg.hip), the same aggregates under a smoothed prolongator (zzz_sagg.hip), aggregates of the node graph under a
// smoothed prolongator that carries the near-nullspace (zzz_sagg_rbm.hip).  mg_coarsen, mg_level_values, mg_restrict and
// mg_prolong are the four places that tell them apart.
enum class MgKind
{
  GEOM,
  PLEVEL,
  AGG,
  SAGG,
  SAGG_RBM
};
static bool mg_smoothed(MgKind k) { return k == MgKind::SAGG || k == MgKind::SAGG_RBM; } // (a stored P whose damping needs the bound)
static bool mg_algebraic(MgKind k) { return k == MgKind::AGG || mg_smoothed(k); }
constexpr int MG_RBM_NODE = 6; // scalar dofs per coarse node of ZZZ_PC_SAGG_RBM: one per rigid-body mode

struct MgLevel
{
  zzz_ctx* ctx = nullptr; // level 0: the caller's; else owned
  MgKind kind = MgKind::GEOM;
  int64_t n[3] = {0, 0, 0}; // cells of the cube (AGG: none)
  int64_t ndof = 0;
  bool slab = false; // level 0 of a hierarchy on several ranks: this rank's planes of the cube, G's window
  int64_t nvec = 0; // entries of this rank's vectors on the level: ndof, but on level 0 of a slab the owned ones
  int order = 1; // PLEVEL: the order of this level's element
  ChebPlan cheb; // the smoother (its vectors: the level context's cheb_g, cheb_d, cheb_d2); the coarsest level has none
  // GEOM: the transfer's tables
  MgGeom G{};
  DevBuf<int32_t> tc, rng;
  DevBuf<double> tf;
  AggLevel* agg = nullptr;   // AGG: the aggregates of this level
  SaggLevel* sagg = nullptr; // SAGG, SAGG_RBM: the aggregates of this level and the prolongator on them
  ~MgLevel()
  {
    agg_free(agg);
    sagg_free(sagg);
  }
};

// what the levels were built from, and what their values were computed from: a set-up compares these
struct MgStructKey
{
  uint64_t feed_version = 0, pattern_version = 0, bc_version = 0; // (pattern and Dirichlet set: the aggregates depend on both)
  int opt_levels = 0, limit = 0;
  MgKind kind = MgKind::GEOM; // of level 0
  int products = 0;           // SAGG, SAGG_RBM: zzz_mg_products' mode; else 0
  int nparts = 1, part = 0;   // GEOM on several ranks: the slab that level 0 is
  bool operator==(const MgStructKey& k) const
  {
    return feed_version == k.feed_version && pattern_version == k.pattern_version && bc_version == k.bc_version
           && opt_levels == k.opt_levels && limit == k.limit && kind == k.kind && products == k.products && nparts == k.nparts
           && part == k.part;
  }
};
struct MgValuesKey
{
  uint64_t mat_version = ~0ull;
  int degree = 2;
  double ratio = 10.0;
  int est_its = 0;
  bool operator==(const MgValuesKey& k) const
  {
    return mat_version == k.mat_version && degree == k.degree && ratio == k.ratio && est_its == k.est_its;
  }
};

struct MgHier
{
  std::vector<std::unique_ptr<MgLevel>> lv;
  DevBuf<double> ainv, tx_in, tx_out;
  MgStructKey skey;
  MgValuesKey vkey;
  int setups = 0;
  bool slab = false;      // level 0 is a z-slab of the cube, the coarser levels are whole on every rank
  double nnz0 = 0.0;      // slab: the nonzeros of the whole cube's matrix (the ranks' owned rows together)
  double coarse_bytes = 0.0;
  double setup_ms = 0.0; // host time of the last set-up that did work (it ends synchronised)
  double cycle_ms = 0.0; // HIP-event time per V-cycle in the last solve with zzz_solver_opts.profile set
  std::vector<hipEvent_t> ev;
  int nev = 0;
  bool ready = false;
  ~MgHier()
  {
    for (hipEvent_t e : ev)
      (void)hipEventDestroy(e);
    for (size_t l = 1; l < lv.size(); ++l)
      if (lv[l]->ctx)
        zzz_ctx_destroy(lv[l]->ctx);
  }
};

constexpr int MG_MAX_LEVELS = 12;
constexpr int64_t MG_DENSE_MAX = 4096; // dofs the dense coarsest solve takes (128 MiB of inverse)

void mg_destroy(zzz_ctx* ctx)
{
  delete ctx->mg;
  ctx->mg = nullptr;
}
int mg_level0_products(const zzz_ctx* ctx)
{
  if (!ctx->mg || !ctx->mg->ready)
    return 0;
  return ctx->mg->lv.size() > 1 ? 2 * ctx->mg->vkey.degree : 0; // degree - 1 terms, the residual, A x of the post-smoother, degree - 1 terms
}
double mg_level0_bound(const zzz_ctx* ctx) { return ctx->mg && ctx->mg->ready ? ctx->mg->lv[0]->cheb.hi : 0.0; }

// The hierarchy belongs to a problem that is gone (zzz_mesh_upload): not ready, so that the zzz_mg_* entry points decline it and
// the next set-up builds anew.  Nothing is freed here (hipFree waits for the whole device); the rebuild or the context frees it.
void mg_invalidate(zzz_ctx* ctx)
{
  if (ctx->mg)
    ctx->mg->ready = false;
}

int mg_check(zzz_ctx* ctx, const zzz_solver_opts* o)
{
  const bool pmg = o->pc == ZZZ_PC_PMG, rbm = o->pc == ZZZ_PC_SAGG_RBM, sagg = o->pc == ZZZ_PC_SAGG;
  const bool agg = o->pc == ZZZ_PC_AGG || sagg || rbm;
  const char* tag = rbm ? "-pc_type sagg_rbm" : sagg ? "-pc_type sagg" : agg ? "-pc_type agg" : pmg ? "-pc_type pmg" : "-pc_type mg";
  if (o->variant == ZZZ_CG_PIPE)
    return fail(ctx, ZZZ_ERR_ARG, "%s: not with -ksp_type pipecg (ZZZ_CG_PIPE takes jacobi or none)", tag);
  if (o->variant != ZZZ_CG_PETSC)
    return fail(ctx, ZZZ_ERR_ARG, "%s: KSPCG (ZZZ_CG_PETSC) only; src/cg.h (ZZZ_CG_CGH) has no preconditioner", tag);
  if (o->single_reduction)
    return fail(ctx, ZZZ_ERR_ARG, "%s: not with -ksp_cg_single_reduction (the classical form of KSPCG only)", tag);
  if (o->op != ZZZ_OP_CSR)
    return fail(ctx, ZZZ_ERR_ARG, "%s: needs the assembled operator, not ZZZ_OP_MATFREE", tag);
  // a communicator: ZZZ_PC_MG alone serves one, of two ranks or more (level 0 on the slabs, the coarser levels whole on every rank)
  int nranks = 1;
  const int rank = comm_rank_of(ctx, &nranks);
  const bool slab = ctx->comm && o->pc == ZZZ_PC_MG && nranks >= 2;
  if (ctx->comm && !slab)
    return fail(ctx, ZZZ_ERR_ARG, "%s: a communicator is attached; multi-rank multigrid is not built", tag);
  if (slab && !comm_has_transport(ctx))
    return fail(ctx, ZZZ_ERR_ARG, "%s: the communicator has no transport (peer-only): the all-reduce of the level-1 right-hand side "
                                  "needs one (zzz_comm_init or zzz_comm_init_local)", tag);
  if (agg)
  {
    // the matrix alone: whatever feed, order, numbering or source of the values
    if (!ctx->pattern.have_pattern || !ctx->values.have_matrix)
      return fail(ctx, ZZZ_ERR_ARG, "%s: needs a sparsity pattern and matrix values", tag);
    if (ctx->n_ghost != 0)
      return fail(ctx, ZZZ_ERR_ARG, "%s: the context has %lld ghost dofs: one rank only", tag, (long long)ctx->n_ghost);
    if (ctx->bs != 1 && ctx->bs != 3)
      return fail(ctx, ZZZ_ERR_ARG, "%s: block size %d", tag, ctx->bs);
    if (rbm && ctx->bs != 3)
      return fail(ctx, ZZZ_ERR_ARG, "%s: block size %d; the rigid-body modes belong to block size 3 -- for scalar problems use "
                                    "-pc_type sagg", tag, ctx->bs);
    if (rbm && ctx->dofmap.near_null_ld == 0)
      return fail(ctx, ZZZ_ERR_ARG, "%s: the context has no near-nullspace: build it with zzz_near_nullspace_build (after the "
                                    "last dofmap upload)", tag);
  }
  else
  {
    if (!ctx->cube_feed)
      return fail(ctx, ZZZ_ERR_ARG, "%s: the feed was uploaded (unstructured or host-built), not generated by "
                                    "zzz_cube_generate: the library does not know the cube to coarsen", tag);
    if (slab && (ctx->cube_nparts != nranks || ctx->cube_part != rank))
      return fail(ctx, ZZZ_ERR_ARG, "%s: the cube was generated as part %d of %d, the communicator has rank %d of %d: a rank's level 0 "
                                    "is its own slab of as many slabs as ranks", tag, ctx->cube_part, ctx->cube_nparts, rank, nranks);
    if (slab && ctx->cube_n[2] < nranks) // (zzz_cube_generate refuses it already)
      return fail(ctx, ZZZ_ERR_ARG, "%s: %lld cell layers for %d ranks: a rank would own none", tag, (long long)ctx->cube_n[2], nranks);
    if (!slab && (ctx->cube_nparts != 1 || ctx->n_ghost != 0))
      return fail(ctx, ZZZ_ERR_ARG, "%s: the cube was generated as part of %d: one part only", tag, ctx->cube_nparts);
    if (ctx->dofmap.order != 1 && !pmg)
      return fail(ctx, ZZZ_ERR_ARG, "%s: order %d; P1 only (p-coarsening for P2 / P3 is -pc_type pmg, ZZZ_PC_PMG)", tag, ctx->dofmap.order);
    if (ctx->dofmap.order < 1 || ctx->dofmap.order > 3)
      return fail(ctx, ZZZ_ERR_ARG, "%s: order %d", tag, ctx->dofmap.order);
    if (ctx->dofmap.order > 1 && o->pc_mg_levels == 1)
      return fail(ctx, ZZZ_ERR_ARG, "%s: pc_mg_levels = 1 at order %d: the P%d level and the P1 level of the same cube make two at least",
                  tag, ctx->dofmap.order, ctx->dofmap.order);
    if (ctx->dofmap.renumbered)
      return fail(ctx, ZZZ_ERR_ARG, "%s: the context keeps an internal dof order; the transfer needs the lexicographic one", tag);
    if (!ctx->values.have_matrix)
      return fail(ctx, ZZZ_ERR_ARG, "%s: matrix not assembled", tag);
  }
  if (o->pc_degree < 0 || o->pc_degree > 64 || o->pc_esteig_its > 64)
    return fail(ctx, ZZZ_ERR_ARG, "%s: smoother degree 1..64, estimate <= 64 steps", tag);
  if (o->pc_mg_levels < 0 || o->pc_mg_coarse_eq_limit < 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: negative pc_mg_levels or pc_mg_coarse_eq_limit", tag);
  return ZZZ_OK;
}

// the error of a child context becomes the caller's
static int child_fail(zzz_ctx* ctx, zzz_ctx* c, int rc, int level, const char* what)
{
  return fail(ctx, rc, "-pc_type mg / pmg / agg / sagg / sagg_rbm, level %d, %s: %s", level, what, c ? c->err.c_str() : zzz_last_error(nullptr));
}

// (slab: F is level 0 of a hierarchy on several ranks -- the window is the planes this rank owns)
static int mg_build_tables(zzz_ctx* ctx, MgLevel& F, const MgLevel& C, bool slab)
{
  int64_t nf_tot = 0, nc_tot = 0, z0 = 0, z1 = F.n[2];
  mg_table_sizes(F.n, C.n, &nf_tot, &nc_tot);
  if ((F.slab = slab))
    mg_slab_planes(F.n[2], ctx->cube_nparts, ctx->cube_part, &z0, &z1);
  std::vector<int32_t> tc((size_t)nf_tot), rng(2 * (size_t)nc_tot);
  std::vector<double> tf((size_t)nf_tot);
  mg_fill_tables(F.G, F.n, C.n, ctx->bs, z0, z1, tc.data(), tf.data(), rng.data());
  if (F.G.nfv * ctx->bs != F.nvec)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type mg: the context owns %lld dofs, planes %lld..%lld of the cube hold %lld", (long long)F.nvec,
                (long long)z0, (long long)z1, (long long)(F.G.nfv * ctx->bs));
  hipStream_t s = ctx->stream;
  ZZZ_HIP(ctx, F.tc.alloc(tc.size()));
  ZZZ_HIP(ctx, F.tf.alloc(tf.size()));
  ZZZ_HIP(ctx, F.rng.alloc(rng.size()));
  ZZZ_HIP(ctx, hipMemcpyAsync(F.tc.p, tc.data(), tc.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ZZZ_HIP(ctx, hipMemcpyAsync(F.tf.p, tf.data(), tf.size() * sizeof(double), hipMemcpyHostToDevice, s));
  ZZZ_HIP(ctx, hipMemcpyAsync(F.rng.p, rng.data(), rng.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (the staging vectors are locals)
  return ZZZ_OK;
}

// The coarsest matrix, downloaded once per set-up, factorised A = L L^T inside its band and inverted column by column
// on the host (plain C++; the columns are independent, so the threads change no bit), symmetrised, uploaded.
static int mg_dense_inverse(zzz_ctx* ctx, MgHier& H)
{
  zzz_ctx* c = H.lv.back()->ctx;
  const int64_t n = c->n_owned * c->bs, nnz = c->nnz;
  std::vector<rp_t> rp((size_t)n + 1);
  std::vector<int32_t> cols((size_t)nnz);
  std::vector<double> vals((size_t)nnz);
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ZZZ_HIP(ctx, hipMemcpy(rp.data(), c->rowptr.p, rp.size() * sizeof(rp_t), hipMemcpyDeviceToHost));
  ZZZ_HIP(ctx, hipMemcpy(cols.data(), c->cols.p, cols.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  ZZZ_HIP(ctx, hipMemcpy(vals.data(), c->vals.p, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> L((size_t)(n * n), 0.0), LT((size_t)(n * n), 0.0), X((size_t)(n * n), 0.0);
  int64_t bw = 0;
  for (int64_t i = 0; i < n; ++i)
    for (rp_t k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k)
    {
      const int64_t j = cols[(size_t)k];
      if (j <= i && vals[(size_t)k] != 0.0)
      {
        L[(size_t)(i * n + j)] = vals[(size_t)k];
        bw = std::max(bw, i - j);
      }
    }
  for (int64_t i = 0; i < n; ++i)
  {
    const int64_t j0 = std::max<int64_t>(0, i - bw);
    for (int64_t j = j0; j <= i; ++j)
    {
      double sum = L[(size_t)(i * n + j)];
      const double *li = &L[(size_t)(i * n)], *lj = &L[(size_t)(j * n)];
      for (int64_t k = std::max(j0, std::max<int64_t>(0, j - bw)); k < j; ++k)
        sum -= li[k] * lj[k];
      if (j == i)
      {
        if (!(sum > 0.0) || !std::isfinite(sum))
          return fail(ctx, ZZZ_ERR_ARG, "-pc_type mg: the coarsest matrix (%lld dofs) is not positive definite: pivot %g in row %lld",
                      (long long)n, sum, (long long)i);
        L[(size_t)(i * n + i)] = std::sqrt(sum);
      }
      else
        L[(size_t)(i * n + j)] = sum / L[(size_t)(j * n + j)];
    }
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = std::max<int64_t>(0, i - bw); j <= i; ++j)
      LT[(size_t)(j * n + i)] = L[(size_t)(i * n + j)];
#pragma omp parallel for schedule(dynamic, 8)
  for (int64_t col = 0; col < n; ++col)
  {
    double* x = &X[(size_t)(col * n)]; // column `col` of the inverse, stored as a row
    // L y = e_col (y is zero above col), then L^T x = y
    for (int64_t i = col; i < n; ++i)
    {
      double sum = i == col ? 1.0 : 0.0;
      const double* li = &L[(size_t)(i * n)];
      for (int64_t k = std::max(col, i - bw); k < i; ++k)
        sum -= li[k] * x[k];
      x[i] = sum / li[i];
    }
    for (int64_t i = n - 1; i >= 0; --i)
    {
      double sum = x[i];
      const double* lt = &LT[(size_t)(i * n)];
      const int64_t k1 = std::min(n - 1, i + bw);
      for (int64_t k = i + 1; k <= k1; ++k)
        sum -= lt[k] * x[k];
      x[i] = sum / lt[i];
    }
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < i; ++j)
    {
      const double v = 0.5 * (X[(size_t)(i * n + j)] + X[(size_t)(j * n + i)]);
      X[(size_t)(i * n + j)] = X[(size_t)(j * n + i)] = v;
    }
  ZZZ_HIP(ctx, H.ainv.reserve((size_t)(n * n)));
  ZZZ_HIP(ctx, hipMemcpy(H.ainv.p, X.data(), X.size() * sizeof(double), hipMemcpyHostToDevice));
  return ZZZ_OK;
}

// a child context on the caller's stream: the cycle needs no event between levels
static int mg_child_create(zzz_ctx* ctx, int level, zzz_ctx** out)
{
  zzz_ctx* c = nullptr;
  if (int rc = zzz_ctx_create(ctx->device, &c))
    return child_fail(ctx, nullptr, rc, level, "context");
  (void)hipStreamDestroy(c->stream);
  c->stream = ctx->stream;
  c->stream_borrowed = true;
  *out = c;
  return ZZZ_OK;
}

// omega of ZZZ_PC_SAGG's prolongator from the bound of the level's smoother
static double mg_omega(const MgLevel& L) { return 4.0 / (3.0 * L.cheb.hi); }

// The next coarser level below the last one, by that level's kind: its context with a pattern (AGG, SAGG: with its values
// too, the Galerkin sums make both; SAGG takes the level's spectrum bound first, by the options os) and the transfer between
// the two.  *more stays false when the kind has none to give: a cube of two cells per axis, or an aggregation that reduces
// the dofs by less than a factor of 2.
static int mg_coarsen(zzz_ctx* ctx, MgHier& H, const zzz_solver_opts* os, bool* more)
{
  MgLevel& F = *H.lv.back();
  const int l = (int)H.lv.size();
  int64_t ncdof = 0;
  if (mg_algebraic(F.kind))
  {
    if (F.kind == MgKind::AGG)
      F.agg = agg_new();
    else
      F.sagg = sagg_new();
    if (int rc = F.agg                         ? agg_aggregate(ctx, F.ctx, F.agg)
                 : F.kind == MgKind::SAGG_RBM ? srbm_aggregate(ctx, F.ctx, F.sagg, l - 1)
                                              : sagg_aggregate(ctx, F.ctx, F.sagg))
      return rc;
    ncdof = F.agg ? agg_count(F.agg) * ctx->bs : sagg_count(F.sagg) * (F.kind == MgKind::SAGG_RBM ? MG_RBM_NODE : ctx->bs);
    if (ncdof == 0 || 2 * ncdof > F.ndof)
    {
      agg_free(F.agg);
      sagg_free(F.sagg);
      F.agg = nullptr;
      F.sagg = nullptr;
      return ZZZ_OK;
    }
  }
  else if (F.kind == MgKind::GEOM && F.n[0] <= 2 && F.n[1] <= 2 && F.n[2] <= 2)
    return ZZZ_OK;
  H.lv.emplace_back(new MgLevel()); // (in the hierarchy before it owns a context: every exit path destroys it)
  MgLevel& C = *H.lv.back();
  C.kind = mg_algebraic(F.kind) ? F.kind : MgKind::GEOM;
  if (int rc = mg_child_create(ctx, l, &C.ctx))
    return rc;
  zzz_ctx* c = C.ctx;
  *more = true;
  if (mg_algebraic(F.kind))
  {
    C.ndof = C.nvec = ncdof;
    // (no block-window product on a level without coordinates; the other forms are packed from the CSR alone)
    c->knob.sellp_bwin = 0;
    if (F.kind == MgKind::AGG)
      return agg_galerkin(ctx, F.ctx, F.agg, c);
    if (int rc = chebyshev_setup(F.ctx, os, F.cheb)) // (kept per set of matrix values: the set-up below finds it again)
      return l > 1 ? child_fail(ctx, F.ctx, rc, l - 1, "spectrum bound") : rc;
    if (F.kind == MgKind::SAGG_RBM)
      return srbm_galerkin(ctx, F.ctx, F.sagg, l > 1 ? H.lv[(size_t)l - 2]->sagg : nullptr, mg_omega(F), c, l - 1);
    return sagg_galerkin(ctx, F.ctx, F.sagg, mg_omega(F), c, l - 1);
  }
  // the same problem re-discretised at order 1: on the same cells below the Pk level, on half of them below a P1 level
  for (int a = 0; a < 3; ++a)
    C.n[a] = F.kind == MgKind::PLEVEL ? F.n[a] : std::max<int64_t>(2, (F.n[a] + 1) / 2);
  C.ndof = C.nvec = (C.n[0] + 1) * (C.n[1] + 1) * (C.n[2] + 1) * ctx->bs;
  if (int rc = zzz_cube_generate(c, ctx->cube_problem, 1, C.n[0], C.n[1], C.n[2], 1, 0, nullptr))
    return child_fail(ctx, c, rc, l, "generate");
  if (int rc = zzz_csr_pattern_build(c))
    return child_fail(ctx, c, rc, l, "pattern");
  if (c->dofmap.renumbered || c->n_owned * c->bs != C.ndof)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type mg / pmg, level %d: the generated level is not in lexicographic order", l);
  return F.kind == MgKind::GEOM ? mg_build_tables(ctx, F, C, H.slab && l == 1) : ZZZ_OK;
}

// level C's matrix values (F: the level above it; built: the levels are new)
static int mg_level_values(zzz_ctx* ctx, MgLevel& F, MgLevel& C, int l, bool built)
{
  if (mg_algebraic(F.kind))
  {
    // (a build has just summed them; a refresh sums the new values on the kept aggregates, level by level -- SAGG with the
    // bound that the level above has just been given)
    if (!built)
      if (int rc = F.agg                         ? agg_refresh(ctx, F.ctx, F.agg, C.ctx)
                   : F.kind == MgKind::SAGG_RBM ? srbm_refresh(ctx, F.ctx, F.sagg, mg_omega(F), C.ctx)
                                                : sagg_refresh(ctx, F.ctx, F.sagg, mg_omega(F), C.ctx))
        return child_fail(ctx, C.ctx, rc, l, "coarse values");
    return ZZZ_OK;
  }
  if (int rc = zzz_assemble_matrix(C.ctx, ctx->cube_problem))
    return child_fail(ctx, C.ctx, rc, l, "assembly");
  return ZZZ_OK;
}

// Level 0 is the caller's context; then coarser levels until one is small enough, the level limit is reached or the kind
// has none to give.  ZZZ_PC_PMG at order > 1: the Pk level first, then the P1 levels from the same cube on; pc_mg_levels
// counts all, and the Pk level is never the coarsest (mg_check refuses pc_mg_levels = 1 there).
static int mg_build(zzz_ctx* ctx, MgHier& H, MgKind kind, const zzz_solver_opts* os, int limit, int max_levels)
{
  const bool agg = mg_algebraic(kind);
  H.lv.emplace_back(new MgLevel());
  MgLevel& L0 = *H.lv[0];
  L0.ctx = ctx;
  L0.ndof = L0.nvec = ctx->n_owned * ctx->bs;
  L0.kind = kind;
  if (!agg) // (to the aggregates the element's order and the cube say nothing)
  {
    L0.order = ctx->dofmap.order;
    for (int a = 0; a < 3; ++a)
      L0.n[a] = ctx->cube_n[a];
    // (a slab: the level rule counts the dofs of the whole cube, so every rank builds the table the one-rank run builds)
    if (H.slab)
      L0.ndof = (L0.n[0] + 1) * (L0.n[1] + 1) * (L0.n[2] + 1) * ctx->bs;
  }
  for (bool more = true; more;)
  {
    const MgLevel& L = *H.lv.back();
    if (L.kind != MgKind::PLEVEL && (L.ndof <= limit || (int)H.lv.size() >= max_levels))
      break;
    more = false;
    if (int rc = mg_coarsen(ctx, H, os, &more))
      return rc;
  }
  const int64_t dofs = H.lv.back()->ndof;
  if (H.slab && H.lv.size() == 1)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type mg: the whole cube (%lld dofs) is a hierarchy of one level, a dense solve of a matrix that no "
                                  "rank of a partition holds: use one rank, or a lower pc_mg_coarse_eq_limit", (long long)dofs);
  if (dofs > MG_DENSE_MAX)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type %s: the coarsest of %d levels has %lld dofs, the dense solve takes at most %lld: "
                                  "allow more levels (pc_mg_levels) or a lower pc_mg_coarse_eq_limit",
                kind == MgKind::SAGG_RBM ? "sagg_rbm" : kind == MgKind::SAGG ? "sagg" : agg ? "agg" : "mg", (int)H.lv.size(), (long long)dofs, (long long)MG_DENSE_MAX);
  return ZZZ_OK;
}

// Several ranks: no rank goes on while another has failed.  Every rank that passed mg_check (whose refusals depend on what
// all ranks share) comes here with its status at the same places of the set-up -- behind the levels, which no collective
// builds, and behind the values -- and leaves with the ranks' common one.  One double through the all-reduce of the CG scalars.
static int mg_agree(zzz_ctx* ctx, int rc, const char* what)
{
  if (!ctx->comm)
    return rc;
  const std::string mine = ctx->err;
  double st = rc ? 1.0 : 0.0;
  int rc2 = comm_inproc_meet(ctx);
  if (!rc2)
    rc2 = comm_allgather_max(ctx, &st);
  if (rc)
  {
    ctx->err = mine;
    return rc;
  }
  if (rc2)
    return rc2;
  if (st != 0.0)
  {
    mg_invalidate(ctx);
    return fail(ctx, ZZZ_ERR_RCCL, "-pc_type mg: another rank failed in the set-up (%s); this rank's hierarchy is dropped with it", what);
  }
  return ZZZ_OK;
}

int mg_setup(zzz_ctx* ctx, const zzz_solver_opts* o)
{
  if (int rc = mg_check(ctx, o))
    return rc;
  const MgKind kind = o->pc == ZZZ_PC_SAGG_RBM ? MgKind::SAGG_RBM : o->pc == ZZZ_PC_SAGG ? MgKind::SAGG : o->pc == ZZZ_PC_AGG ? MgKind::AGG
                      : ctx->dofmap.order > 1 ? MgKind::PLEVEL : MgKind::GEOM;
  const bool agg = mg_algebraic(kind);
  const int limit = o->pc_mg_coarse_eq_limit > 0 ? o->pc_mg_coarse_eq_limit : 1000;
  const int max_levels = o->pc_mg_levels > 0 ? std::min<int>(o->pc_mg_levels, MG_MAX_LEVELS) : MG_MAX_LEVELS;
  const MgStructKey skey{ctx->feed_version, agg ? ctx->pattern_version : 0, agg ? ctx->bc_version : 0, o->pc_mg_levels, limit, kind,
                         mg_smoothed(kind) ? ctx->mg_products : 0, ctx->comm ? ctx->cube_nparts : 1, ctx->comm ? ctx->cube_part : 0};
  const MgValuesKey vkey{ctx->mat_version, o->pc_degree > 0 ? o->pc_degree : 2, o->pc_ratio > 1.0 ? o->pc_ratio : 10.0,
                         o->pc_esteig_its == 0 ? 10 : o->pc_esteig_its};
  // the options of the levels' spectrum estimates and smoothers
  zzz_solver_opts os = *o;
  os.variant = ZZZ_CG_PETSC;
  os.op = ZZZ_OP_CSR;
  os.single_reduction = 0;
  os.pc_degree = vkey.degree;
  os.pc_ratio = vkey.ratio;
  MgHier* H = ctx->mg;
  bool built = false;
  const auto t_begin = std::chrono::steady_clock::now();
  // (the two halves of the set-up as functions of their own: with a communicator the ranks agree on the status of each, mg_agree)
  auto levels = [&]() -> int {
    if (H && H->ready && H->skey == skey)
      return ZZZ_OK;
    // ---- the levels --------------------------------------------------------------------------
    mg_destroy(ctx);
    size_t free0 = 0, free1 = 0, total = 0;
    ZZZ_HIP(ctx, hipMemGetInfo(&free0, &total));
    H = ctx->mg = new MgHier();
    H->slab = ctx->comm != nullptr; // (mg_check: ZZZ_PC_MG on two ranks or more)
    if (int rc = mg_build(ctx, *H, kind, &os, limit, max_levels))
    {
      mg_destroy(ctx);
      return rc;
    }
    // smoother work vectors of every level that smooths (level 0's as ZZZ_PC_CHEBYSHEV_JACOBI allocates them)
    for (size_t l = 0; l + 1 < H->lv.size(); ++l)
    {
      zzz_ctx* c = H->lv[l]->ctx;
      ZZZ_HIP(ctx, c->cheb_d.alloc((size_t)c->nloc()));
      ZZZ_HIP(ctx, c->cheb_d2.alloc((size_t)c->nloc()));
      ZZZ_HIP(ctx, c->cheb_g.alloc((size_t)c->nloc()));
    }
    ZZZ_HIP(ctx, hipMemGetInfo(&free1, &total));
    H->coarse_bytes = free0 > free1 ? (double)(free0 - free1) : 0.0; // (set-up scratch of the levels included; level 0's smoother vectors too)
    H->skey = skey; // (H->vkey: of no matrix yet)
    built = true;
    return ZZZ_OK;
  };
  if (int rc = mg_agree(ctx, levels(), "the levels"))
  {
    mg_destroy(ctx);
    return rc;
  }
  H = ctx->mg;
  auto values_of_levels = [&]() -> int {
    if (H->vkey == vkey)
      return ZZZ_OK;
    // (SAGG: the bounds are part of the prolongator, so another estimate is other values)
    const bool values = H->vkey.mat_version != vkey.mat_version || (mg_smoothed(kind) && H->vkey.est_its != vkey.est_its);
    H->ready = false;
    // ---- the levels' values: matrices, inverse diagonals, spectrum bounds, the coarsest inverse ----
    for (size_t l = 0; l < H->lv.size(); ++l)
    {
      MgLevel& L = *H->lv[l];
      zzz_ctx* c = L.ctx;
      if (l > 0 && values)
        if (int rc = mg_level_values(ctx, *H->lv[l - 1], L, (int)l, built))
          return rc;
      L.cheb = ChebPlan();
      if (l + 1 == H->lv.size())
        break;
      if (int rc = chebyshev_setup(c, &os, L.cheb)) // (the level's own bound; leaves c->dinv = 1 / diag(A))
        return l > 0 ? child_fail(ctx, c, rc, (int)l, "spectrum bound") : rc;
      L.cheb.fused = false; // (a level's product and term stay two launches)
    }
    if (values)
      if (int rc = mg_dense_inverse(ctx, *H))
        return rc;
    H->vkey = vkey;
    ++H->setups;
    H->ready = true;
    ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    H->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return ZZZ_OK;
  };
  if (int rc = mg_agree(ctx, values_of_levels(), "the levels' values"))
    return rc;
  // (a slab: the nonzeros of the whole cube's matrix for zzz_mg_info -- the owned rows of the ranks together; collective)
  if (H->slab)
  {
    int nranks = 1;
    comm_rank_of(ctx, &nranks);
    std::vector<double> all((size_t)nranks, 0.0);
    if (int rc = comm_allgather_double(ctx, (double)ctx->nnz, all.data()))
      return rc;
    H->nnz0 = 0.0;
    for (double v : all)
      H->nnz0 += v;
  }
  // the estimates above ran Jacobi solves through the levels' vectors: the inverse diagonals as the cycle reads them
  for (size_t l = 0; l + 1 < H->lv.size(); ++l)
  {
    zzz_ctx* c = H->lv[l]->ctx;
    cg_launch_extract_dinv(c, c->n_owned * c->bs, 1);
  }
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

static int mg_restrict(zzz_ctx* ctx, const int* stop, MgLevel& F, MgLevel& C, const double* rf, const double* sub, double* rc)
{
  switch (F.kind)
  {
  case MgKind::AGG:
    return agg_restrict(ctx, stop, F.agg, F.ctx->bc.p, rf, sub, rc);
  case MgKind::SAGG:
  case MgKind::SAGG_RBM:
    return sagg_restrict(ctx, stop, F.sagg, rf, sub, rc);
  case MgKind::PLEVEL:
    return pmg_restrict(ctx, stop, F.order, ctx->bs, F.n, F.ctx->bc.p, C.ctx->bc.p, rf, sub, rc);
  case MgKind::GEOM:
    break;
  }
  const int g = vgrid(F.G.ncv * 8); // (a thread walks up to 64 fine vertices: one coarse vertex per thread, no striding)
  if (ctx->bs == 3)
    hipLaunchKernelGGL(k_mg_restrict<3>, dim3(g), dim3(VB), 0, ctx->stream, stop, F.G, F.tc.p, F.tf.p, F.rng.p, F.ctx->bc.p, C.ctx->bc.p,
                       rf, sub, rc);
  else
    hipLaunchKernelGGL(k_mg_restrict<1>, dim3(g), dim3(VB), 0, ctx->stream, stop, F.G, F.tc.p, F.tf.p, F.rng.p, F.ctx->bc.p, C.ctx->bc.p,
                       rf, sub, rc);
  if (!F.slab)
    return ZZZ_OK;
  // a slab's window: the coarse planes it cannot reach are zero, and the ranks' partial sums are added by the communicator, in its
  // order (issued whatever the stop flag says: the ranks stay in step)
  const size_t plane = (size_t)F.G.pc[0] * F.G.pc[1] * ctx->bs, below = (size_t)F.G.cz0 * plane, upto = ((size_t)F.G.cz1 + 1) * plane;
  if (below)
    ZZZ_HIP(ctx, hipMemsetAsync(rc, 0, below * sizeof(double), ctx->stream));
  if (upto < (size_t)C.ndof)
    ZZZ_HIP(ctx, hipMemsetAsync(rc + upto, 0, ((size_t)C.ndof - upto) * sizeof(double), ctx->stream));
  return comm_allreduce_sum(ctx, rc, (int)C.ndof);
}
static int mg_prolong(zzz_ctx* ctx, const int* stop, MgLevel& F, MgLevel& C, const double* ec, double* xf, int accumulate)
{
  switch (F.kind)
  {
  case MgKind::AGG:
    return agg_prolong(ctx, stop, F.agg, F.ctx->bc.p, ec, xf, accumulate);
  case MgKind::SAGG:
  case MgKind::SAGG_RBM:
    return sagg_prolong(ctx, stop, F.sagg, ec, xf, accumulate);
  case MgKind::PLEVEL:
    return pmg_prolong(ctx, stop, F.order, ctx->bs, F.n, F.ctx->bc.p, C.ctx->bc.p, ec, xf, accumulate);
  case MgKind::GEOM:
    break;
  }
  hipLaunchKernelGGL(k_mg_prolong, dim3(vgrid(F.G.nfv * 4)), dim3(VB), 0, ctx->stream, stop, F.G, F.tc.p, F.tf.p, F.ctx->bc.p, C.ctx->bc.p,
                     ec, xf, accumulate);
  return ZZZ_OK;
}

// (the smoother is the polynomial of zzz_cg.hip on the level's context: product and term as separate launches)
static int mg_cycle_level(zzz_ctx* ctx, const int* stop, MgHier& H, size_t l, const double* b, double* x)
{
  MgLevel& L = *H.lv[l];
  zzz_ctx* c = L.ctx;
  if (l + 1 == H.lv.size())
  {
    const int64_t n = c->n_owned * c->bs;
    hipLaunchKernelGGL(k_mg_dense, dim3((unsigned)((n + VB / 64 - 1) / (VB / 64))), dim3(VB), 0, ctx->stream, stop, H.ainv.p, b, x, (int)n);
    return ZZZ_OK;
  }
  MgLevel& C = *H.lv[l + 1];
  double* t = L.cheb.d2;
  // pre-smoother from zero
  cheb_first(c, ctx, L.cheb, b, nullptr, x);
  if (int rc = cheb_terms(c, ctx, L.cheb, b, x))
    return rc;
  // coarse correction: r_c = P~^T (b - A x), e_c = M_c r_c, x += P~ e_c
  if (int rc = launch_product(c, x, t, nullptr, nullptr)) // (level 0 of a slab exchanges the halo of x; else launch_spmv)
    return rc;
  if (int rc = mg_restrict(ctx, stop, L, C, b, t, C.ctx->b.p))
    return rc;
  if (int rc = mg_cycle_level(ctx, stop, H, l + 1, C.ctx->b.p, C.ctx->u.p))
    return rc;
  if (int rc = mg_prolong(ctx, stop, L, C, C.ctx->u.p, x, 1))
    return rc;
  // post-smoother from x: the same polynomial
  if (int rc = launch_product(c, x, t, nullptr, nullptr))
    return rc;
  cheb_first(c, ctx, L.cheb, b, t, x);
  return cheb_terms(c, ctx, L.cheb, b, x);
}

int mg_vcycle(zzz_ctx* ctx, const double* r, double* z, bool timed)
{
  if (!ctx->mg || !ctx->mg->ready)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type mg: no hierarchy (zzz_mg_setup)");
  MgHier& H = *ctx->mg;
  timed = timed && H.nev + 2 <= 64;
  if (timed)
  {
    while ((int)H.ev.size() < H.nev + 2)
    {
      hipEvent_t e;
      ZZZ_HIP(ctx, hipEventCreate(&e));
      H.ev.push_back(e);
    }
    (void)hipEventRecord(H.ev[(size_t)H.nev], ctx->stream);
  }
  if (int rc = mg_cycle_level(ctx, reinterpret_cast<const int*>(ctx->state.p), H, 0, r, z))
    return rc;
  if (timed)
  {
    (void)hipEventRecord(H.ev[(size_t)H.nev + 1], ctx->stream);
    H.nev += 2;
  }
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}
// the cycles of a profiled solve that ran before it stopped: the first `cycles` event pairs (the stream is idle)
void mg_profile_begin(zzz_ctx* ctx)
{
  if (ctx->mg)
    ctx->mg->nev = 0;
}
void mg_profile_end(zzz_ctx* ctx, int cycles)
{
  if (!ctx->mg)
    return;
  MgHier& H = *ctx->mg;
  double sum = 0.0;
  int n = 0;
  for (int i = 0; i < std::min(cycles, H.nev / 2); ++i)
  {
    float ms = 0;
    if (hipEventElapsedTime(&ms, H.ev[2 * (size_t)i], H.ev[2 * (size_t)i + 1]) == hipSuccess)
    {
      sum += ms;
      ++n;
    }
  }
  H.cycle_ms = n ? sum / n : 0.0;
  H.nev = 0;
}
ZZZ_PRELOAD_TU(mg)
} // namespace zzz

using namespace zzz;

extern "C" {

int zzz_mg_setup(zzz_ctx* ctx, const zzz_solver_opts* opts)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  if (!opts)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_setup: NULL options");
  zzz_solver_opts o = *opts;
  o.pc = opts->pc == ZZZ_PC_PMG || opts->pc == ZZZ_PC_AGG || opts->pc == ZZZ_PC_SAGG || opts->pc == ZZZ_PC_SAGG_RBM ? opts->pc : ZZZ_PC_MG;
  if (int rc = mg_setup(ctx, &o))
    return rc;
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZZZ_OK;
}

int zzz_mg_info(zzz_ctx* ctx, int level, double out[8])
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  if (!out)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_info: NULL output");
  for (int i = 0; i < 8; ++i)
    out[i] = 0.0;
  const MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_info: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_MG)");
  if (level < 0)
  {
    out[0] = (double)H->lv.size();
    out[1] = (double)H->lv.back()->ndof;
    out[2] = (double)H->setups;
    out[3] = (double)mg_level0_products(ctx);
    out[4] = H->coarse_bytes;
    out[5] = H->cycle_ms;
    out[6] = H->setup_ms;
    out[7] = H->lv[0]->kind == MgKind::PLEVEL ? 1.0 : 0.0;
    return ZZZ_OK;
  }
  if ((size_t)level >= H->lv.size())
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_info: level %d of %d", level, (int)H->lv.size());
  const MgLevel& L = *H->lv[(size_t)level];
  out[0] = (double)L.n[0];
  out[1] = (double)L.n[1];
  out[2] = (double)L.n[2];
  if (L.kind == MgKind::SAGG_RBM && level > 0) // (no cube: ny's slot holds the dropped coarse dofs among this level's)
    out[1] = (double)srbm_dropped(H->lv[(size_t)level - 1]->sagg);
  out[3] = (double)L.ndof;
  out[4] = level == 0 && H->slab ? H->nnz0 : (double)L.ctx->nnz; // (a slab: the whole cube's, as its cells and dofs are)
  const bool smooths = (size_t)level + 1 < H->lv.size();
  out[5] = smooths ? L.cheb.hi : 0.0;
  out[6] = smooths ? L.cheb.lo : 0.0;
  out[7] = smooths ? (double)L.cheb.degree : 0.0;
  return ZZZ_OK;
}

int zzz_mg_products(zzz_ctx* ctx, int mode)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  if (mode != ZZZ_MG_PRODUCTS_LISTS && mode != ZZZ_MG_PRODUCTS_ROWS)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_products: mode %d (ZZZ_MG_PRODUCTS_LISTS = 0, ZZZ_MG_PRODUCTS_ROWS = 1)", mode);
  ctx->mg_products = mode; // (part of MgStructKey: the next set-up of a smoothed hierarchy compares it)
  return ZZZ_OK;
}

int zzz_mg_products_info(zzz_ctx* ctx, int64_t info[8])
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  if (!info)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_products_info: NULL output");
  for (int i = 0; i < 8; ++i)
    info[i] = 0;
  const MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_products_info: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_SAGG)");
  if (!mg_smoothed(H->lv[0]->kind))
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_products_info: the hierarchy is not ZZZ_PC_SAGG's or ZZZ_PC_SAGG_RBM's: it forms no products");
  info[0] = H->skey.products;
  for (size_t l = 0; l + 1 < H->lv.size(); ++l)
  {
    int64_t li[8];
    if (!H->lv[l]->sagg)
      continue;
    sagg_products_info(H->lv[l]->sagg, li);
    info[1] += li[1];
    info[2] += li[2];
    info[3] = std::max(info[3], li[3]);
    info[4] = std::max(info[4], li[4]);
    info[5] += li[5];
    info[6] = std::max(info[6], li[6]);
  }
  return ZZZ_OK;
}

int zzz_mg_apply(zzz_ctx* ctx, const double* r, double* z)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  if (!r || !z)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_apply: NULL vector");
  if (!ctx->mg || !ctx->mg->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_apply: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_MG)");
  const size_t n = (size_t)(ctx->n_owned * ctx->bs);
  hipStream_t s = ctx->stream;
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->state.p, 0, sizeof(CgState), s)); // (a finished solve leaves its stop flag set)
  // (a context in an internal dof order -- ZZZ_PC_AGG and ZZZ_PC_SAGG alone serve one -- translates at the boundary, as zzz_spmv does)
  std::vector<double> ri, zi;
  if (ctx->dofmap.renumbered)
  {
    ri.resize(n);
    zi.resize(n);
    to_internal(ctx, r, ri.data(), true);
  }
  ZZZ_HIP(ctx, hipMemcpyAsync(ctx->r.p, ctx->dofmap.renumbered ? ri.data() : r, n * sizeof(double), hipMemcpyHostToDevice, s));
  if (int rc = mg_vcycle(ctx, ctx->r.p, ctx->z.p, false))
    return rc;
  ZZZ_HIP(ctx, hipMemcpyAsync(ctx->dofmap.renumbered ? zi.data() : z, ctx->z.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s));
  if (ctx->dofmap.renumbered)
    to_caller(ctx, zi.data(), z, true);
  return ZZZ_OK;
}

int zzz_mg_transfer(zzz_ctx* ctx, int level, int dir, const double* in, double* out)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_transfer: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_MG)");
  if (level < 0 || (size_t)level + 1 >= H->lv.size() || (dir != 0 && dir != 1) || !in || !out)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_transfer: level %d of %d (the coarsest has no transfer below it), dir %d, or NULL vector",
                level, (int)H->lv.size(), dir);
  MgLevel &F = *H->lv[(size_t)level], &C = *H->lv[(size_t)level + 1];
  const size_t nin = (size_t)(dir == 0 ? C.nvec : F.nvec), nout = (size_t)(dir == 0 ? F.nvec : C.nvec);
  hipStream_t s = ctx->stream;
  ZZZ_HIP(ctx, H->tx_in.reserve(nin));
  ZZZ_HIP(ctx, H->tx_out.reserve(nout));
  // (level 0 of a context in an internal dof order: its side of the pair is translated)
  const bool tr = level == 0 && ctx->dofmap.renumbered;
  std::vector<double> vi;
  if (tr && dir == 1)
  {
    vi.resize(nin);
    to_internal(ctx, in, vi.data(), true);
    in = vi.data();
  }
  ZZZ_HIP(ctx, hipMemcpyAsync(H->tx_in.p, in, nin * sizeof(double), hipMemcpyHostToDevice, s));
  if (dir == 0)
  {
    if (int rc = mg_prolong(ctx, nullptr, F, C, H->tx_in.p, H->tx_out.p, 0))
      return rc;
  }
  else if (int rc = mg_restrict(ctx, nullptr, F, C, H->tx_in.p, nullptr, H->tx_out.p))
    return rc;
  ZZZ_HIP(ctx, hipGetLastError());
  if (tr && dir == 0)
    vi.resize(nout);
  ZZZ_HIP(ctx, hipMemcpyAsync(tr && dir == 0 ? vi.data() : out, H->tx_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s));
  if (tr && dir == 0)
    to_caller(ctx, vi.data(), out, true);
  return ZZZ_OK;
}

int zzz_mg_level_csr(zzz_ctx* ctx, int level, int64_t* rowptr, int32_t* cols, double* vals)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_csr: no hierarchy (zzz_mg_setup, or a solve with a multigrid preconditioner)");
  if (level < 1 || (size_t)level >= H->lv.size())
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_csr: level %d; the coarse levels are 1 .. %d (level 0 is zzz_csr_download's)", level,
                (int)H->lv.size() - 1);
  const zzz_ctx* c = H->lv[(size_t)level]->ctx;
  if (c->dofmap.renumbered)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_csr: level %d keeps an internal dof order", level);
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rowptr)
    ZZZ_HIP(ctx, hipMemcpy(rowptr, c->rowptr.p, ((size_t)c->nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (cols)
    ZZZ_HIP(ctx, hipMemcpy(cols, c->cols.p, (size_t)c->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (vals)
    ZZZ_HIP(ctx, hipMemcpy(vals, c->vals.p, (size_t)c->nnz * sizeof(double), hipMemcpyDeviceToHost));
  return ZZZ_OK;
}

int zzz_mg_level_p(zzz_ctx* ctx, int level, int64_t* rowptr, int32_t* cols, double* vals, int64_t* out_nnz)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_p: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_SAGG)");
  if (!mg_smoothed(H->lv[0]->kind))
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_p: the hierarchy is not ZZZ_PC_SAGG's or ZZZ_PC_SAGG_RBM's: no prolongator is stored");
  if (level < 0 || (size_t)level + 1 >= H->lv.size())
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_p: level %d of %d (the coarsest has no prolongator below it)", level, (int)H->lv.size());
  const MgLevel& F = *H->lv[(size_t)level];
  if (out_nnz)
    *out_nnz = sagg_p_nnz(F.sagg);
  return sagg_download_p(ctx, F.ctx, F.sagg, rowptr, cols, vals);
}

int zzz_mg_level_nns(zzz_ctx* ctx, int level, double* out)
{
  if (!ctx)
    return fail(nullptr, ZZZ_ERR_ARG, "NULL context");
  ZZZ_HIP(ctx, hipSetDevice(ctx->device));
  MgHier* H = ctx->mg;
  if (!H || !H->ready)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_nns: no hierarchy (zzz_mg_setup, or a solve with ZZZ_PC_SAGG_RBM)");
  if (H->lv[0]->kind != MgKind::SAGG_RBM)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_nns: the hierarchy is not ZZZ_PC_SAGG_RBM's: no near-nullspace is carried");
  if (level < 0 || (size_t)level >= H->lv.size() || H->lv.size() < 2 || !out)
    return fail(ctx, ZZZ_ERR_ARG, "zzz_mg_level_nns: level %d of %d (a hierarchy of one level orthogonalises nothing), or NULL output",
                level, (int)H->lv.size());
  // level 0's is kept in the caller's numbering; a coarse level reads what the level above wrote
  const double* B = level == 0 ? srbm_nns(H->lv[0]->sagg, false) : srbm_nns(H->lv[(size_t)level - 1]->sagg, true);
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ZZZ_HIP(ctx, hipMemcpy(out, B, (size_t)(MG_RBM_NODE * H->lv[(size_t)level]->ndof) * sizeof(double), hipMemcpyDeviceToHost));
  return ZZZ_OK;
}
}
