// ZZZ_PC_SAGG_RBM: smoothed-aggregation multigrid whose tentative prolongator carries the near-nullspace -- the six rigid-body
// modes of zzz_near_nullspace_build -- through every level (PETSc's -pc_type gamg with MatSetNearNullSpace, what the reference
// builds the modes for: src/elasticity_problem.cpp:233-244).  It is ZZZ_PC_SAGG (zzz_sagg.hip) with another P_t.  This file
// holds what that changes: the near-nullspace of a level, the per-aggregate orthogonalisation, the terms and values of P, the
// node graph of a coarse level and the unit diagonals of dropped coarse dofs.  R = P^T, T = A P, A_c = P^T T, their refresh
// and the two transfers are zzz_sagg.hip's (zzz_sagg.h); aggregation is zzz_agg.hip's; levels, smoother, V-cycle, dense
// coarsest solve, caching and profiling are zzz_mg.hip's.
//
// The rule, per level (tests/_sagg_rbm_ref.py restates it sum for sum).  Scope, options, level rule, smoother, cycle, spectrum
// bound and omega = 4 / (3 hi) are ZZZ_PC_SAGG's.  Every sum is a chain of plain double additions of individually rounded
// products, with no fused multiply-add.
//   node size   3 on level 0, 6 on every coarse level.
//   B           level 0: the library's six vectors as zzz_near_nullspace_build left them, in the caller's numbering, entries of
//               constrained scalar dofs taken as 0.  Level l + 1: the B_c below, 6 columns by 6 rows per aggregate.
//   aggregates  ZZZ_PC_AGG's rule on the node graph of the level's matrix: nodes are blocks of 3 scalar dofs on level 0 and
//               blocks of 6 below.
//   P_t, B_c    per aggregate J, its m member nodes in ascending index (the caller's numbering on level 0): take the rows of B of
//               its member dofs, node-major then component ascending; modified Gram-Schmidt over the six columns in column order
//               q = 0..5: for j < q, R(j, q) = <Q_j, b_q>, then b_q -= R(j, q) Q_j; then R(q, q) = |b_q| and Q_q = b_q / R(q, q).
//               A column is DROPPED when |b_q| after the projections is at most 2^-30 of its norm before them, or when it is
//               zero: then Q_q = 0 and row q of R is 0.  (An exactly dependent column leaves round-off of order 6 x 2^-52
//               relative; an independent one keeps roughly aggregate radius / domain size.)  P_t(row, (J, q)) = Q_q(row); rows
//               of constrained dofs and dropped columns carry no entries.  B_c's rows (J, 0..5) are R.
//   one sum     every inner product and norm: partial sum l (l = 0..63) adds the products of the rows l, l + 64, ... front to
//               back, then the 64 partial sums meet in the tree s[i] += s[i + o] for i < o, o = 32, 16, 8, 4, 2, 1; the result
//               is s[0].  A norm is the square root of that sum of squares.  (A wavefront per aggregate, the shuffle tree of
//               zzz_mg.hip's dense solve.)
//   P           P_t - omega D^-1 (A P_t): P(i, (J, q)) = P_t(i, (J, q)) - (omega s) / a_ii, s = sum_k a_ik P_t(k, (J, q)) over
//               the unconstrained k in ascending k.  Pattern: (i, (J, q)) wherever row i is unconstrained and has a structural
//               a_ik with k unconstrained, k in aggregate J and column q kept.  Rows of constrained dofs are empty.
//   R, T, A_c   R = P^T, T = A P and A_c = P^T T exactly as ZZZ_PC_SAGG forms them: sorted term lists, ascending summation
//               index, one thread per run.
//   dropped     a dropped coarse dof (J, q) has no entry in P; its row of A_c is the single entry 1 on the diagonal.  On the
//               next level it is an ordinary dof with a zero row in B.
// The aggregates, Q, B_c and the drops depend on B, the Dirichlet bytes and the kept aggregates only: new matrix values re-form
// P's values, T and A_c on the kept lists (no orthogonalisation, no sort, no allocation) to the bits of a fresh set-up.
//
// Aggregates have no size cap (hundreds of rows per column are common), so the lanes of the orthogonalisation loop over the
// rows and Q lives in qt -- P_t's value array -- between the passes; a lane only ever reads back rows it wrote itself.  The
// coarse contexts adopt their matrix as scalar (block size 1): the node size belongs to the level, not to the context.
#include "zzz_sagg.h"

namespace zzz
{
// level 0: B[q][caller's index of d] = the library's vector q at the stored dof d, 0 where d is constrained
__global__ __launch_bounds__(VB) void k_srbm_b0(int64_t nf, int64_t ld, const double* __restrict__ nn, const uint8_t* __restrict__ bc,
                                                const int32_t* __restrict__ perm, double* __restrict__ B)
{
  SAGG_FOR(d, nf)
  {
    const int64_t cd = (int64_t)sagg_caller<3>(perm, (int32_t)d);
    const bool fixed = bc[d] != 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
    {
      const double v = nn[q * ld + d];
      B[q * nf + cd] = fixed ? 0.0 : v;
    }
  }
}

// pos[node] = its place in the aggregates' inverted map
__global__ __launch_bounds__(VB) void k_srbm_member_pos(int64_t nn, const int32_t* __restrict__ mem, int32_t* __restrict__ pos)
{
  SAGG_FOR(t, nn)
    pos[mem[t]] = (int32_t)t;
}

// the rows the orthogonalisation reads: qt[q][g] = B[q][caller's index of the dof of member row g], 0 where it is constrained
template <int NS>
__global__ __launch_bounds__(VB) void k_srbm_gather_rows(int64_t nf, const int32_t* __restrict__ mem, const uint8_t* __restrict__ bc,
                                                         const int32_t* __restrict__ perm, const double* __restrict__ B,
                                                         double* __restrict__ qt)
{
  SAGG_FOR(g, nf)
  {
    const int32_t d = mem[g / NS] * NS + (int32_t)(g % NS);
    const int64_t cd = (int64_t)sagg_caller<NS>(perm, d);
    const bool fixed = bc[d] != 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
    {
      const double v = B[q * nf + cd];
      qt[q * nf + g] = fixed ? 0.0 : v;
    }
  }
}

// the rule's one sum: the 64 partial sums meet in the shuffle tree; every lane gets lane 0's result
__device__ inline double srbm_wave_sum(double acc)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    acc += __shfl_down(acc, o, 64);
  return __shfl(acc, 0, 64);
}

// Modified Gram-Schmidt of the six columns of an aggregate's rows, a wavefront per aggregate: lane l owns the member rows
// g0 + l, g0 + l + 64, ...; Q replaces B in qt column by column; R goes to the next level's B (row (J, j), column q) and the
// drops to drop[6 J + q].  No lane reads a row another lane wrote: the only exchange is the shuffle tree.
__global__ __launch_bounds__(VB) void k_srbm_qr(int64_t nagg, int ns, int64_t nf, int64_t nc, const int32_t* __restrict__ moff,
                                                double* qt, double* __restrict__ Bc, int32_t* __restrict__ drop)
{
  const int lane = threadIdx.x & 63;
  for (int64_t J = blockIdx.x * (int64_t)(VB / 64) + (threadIdx.x >> 6); J < nagg; J += (int64_t)gridDim.x * (VB / 64))
  {
    const int64_t g0 = (int64_t)moff[J] * ns, g1 = (int64_t)moff[J + 1] * ns;
    unsigned kept = 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
    {
      double* bq = qt + q * nf;
      double acc = 0.0;
      for (int64_t g = g0 + lane; g < g1; g += 64)
      {
        const double v = bq[g];
        acc += v * v;
      }
      const double before = sqrt(srbm_wave_sum(acc));
#pragma unroll
      for (int j = 0; j < q; ++j)
      {
        double r = 0.0;
        if ((kept >> j) & 1u) // (the same in every lane)
        {
          const double* qj = qt + j * nf;
          acc = 0.0;
          for (int64_t g = g0 + lane; g < g1; g += 64)
          {
            const double a = qj[g], b = bq[g];
            acc += a * b;
          }
          r = srbm_wave_sum(acc);
          for (int64_t g = g0 + lane; g < g1; g += 64)
          {
            const double a = qj[g], b = bq[g];
            bq[g] = b - r * a;
          }
        }
        if (lane == 0)
          Bc[q * nc + J * RBM_NCOL + j] = r;
      }
      acc = 0.0;
      for (int64_t g = g0 + lane; g < g1; g += 64)
      {
        const double v = bq[g];
        acc += v * v;
      }
      const double after = sqrt(srbm_wave_sum(acc));
      const bool keep = !(after == 0.0 || after <= 0x1p-30 * before);
      for (int64_t g = g0 + lane; g < g1; g += 64)
      {
        const double v = bq[g];
        bq[g] = keep ? v / after : 0.0;
      }
      kept |= (keep ? 1u : 0u) << q;
      if (lane == 0)
      {
        Bc[q * nc + J * RBM_NCOL + q] = keep ? after : 0.0;
#pragma unroll
        for (int j = q + 1; j < RBM_NCOL; ++j)
          Bc[q * nc + J * RBM_NCOL + j] = 0.0;
        drop[J * RBM_NCOL + q] = keep ? 0 : 1;
      }
    }
  }
}

// the dropped coarse dofs, ascending: list[scan[d]] = d
__global__ __launch_bounds__(VB) void k_srbm_drop_list(int64_t nc, const int32_t* __restrict__ drop, const int32_t* __restrict__ scan,
                                                       int32_t* __restrict__ list)
{
  SAGG_FOR(d, nc)
    if (drop[d])
      list[scan[d]] = (int32_t)d;
}

// terms of P that matrix entry order[t] (order null: t) brings: the kept columns of the aggregate of its column, where row and
// column are unconstrained
template <int NS>
__global__ __launch_bounds__(VB) void k_srbm_p_count(int64_t nnz, const u64* __restrict__ order, const int32_t* __restrict__ rowidx,
                                                     const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                     const int32_t* __restrict__ agg, const int32_t* __restrict__ drop,
                                                     int32_t* __restrict__ cnt)
{
  SAGG_FOR(t, nnz)
  {
    const int32_t k = order ? (int32_t)order[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    const int32_t J = agg[c / NS];
    const bool ok = J >= 0 && bc[r] == 0 && bc[c] == 0;
    const int64_t o = (int64_t)(J >= 0 ? J : 0) * RBM_NCOL;
    int32_t n = 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
      n += drop[o + q] ? 0 : 1;
    cnt[t] = ok ? n : 0;
    if (t == 0)
      cnt[nnz] = 0;
  }
}
// ... written out: key (stored row, coarse dof (J, q)), value (matrix entry, place of P_t(column, (J, q)) in qt)
template <int NS>
__global__ __launch_bounds__(VB) void k_srbm_p_terms(int64_t nnz, int64_t nf, const u64* __restrict__ order, const int32_t* __restrict__ rowidx,
                                                     const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                     const int32_t* __restrict__ agg, const int32_t* __restrict__ drop,
                                                     const int32_t* __restrict__ pos, const int64_t* __restrict__ off,
                                                     u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(t, nnz)
  {
    const int32_t k = order ? (int32_t)order[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    const int32_t J = agg[c / NS];
    if (J < 0 || bc[r] != 0 || bc[c] != 0)
      continue;
    const u64 g = (u64)pos[c / NS] * NS + (unsigned)(c % NS);
    int64_t o = off[t];
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
      if (!drop[(int64_t)J * RBM_NCOL + q])
      {
        key[o] = ((u64)r << 32) | ((u64)J * RBM_NCOL + (unsigned)q);
        val[o] = ((u64)k << 32) | ((u64)q * (u64)nf + g);
        ++o;
      }
  }
}

// P(i, (J, q)) = P_t(i, (J, q)) - (omega s) / a_ii, s the run's products a_ik P_t(k, (J, q)) summed front to back.  P_t(i, (J, q))
// is row i's own place in qt when i belongs to J, else 0: loaded at that (always valid) place either way, then selected.
template <int NS>
__global__ __launch_bounds__(VB) void k_srbm_p_values(int64_t pnnz, int64_t nf, const int32_t* __restrict__ pseg, const u64* __restrict__ psrc,
                                                      const double* __restrict__ a, const double* __restrict__ qt,
                                                      const int32_t* __restrict__ pfrow, const int32_t* __restrict__ pcol,
                                                      const int32_t* __restrict__ agg, const int32_t* __restrict__ pos,
                                                      const double* __restrict__ diag, double omega, double* __restrict__ pval)
{
  SAGG_FOR(e, pnnz)
  {
    double s = 0.0;
    for (int32_t t = pseg[e]; t < pseg[e + 1]; ++t)
    {
      const u64 p = psrc[t];
      s += a[p >> 32] * qt[p & 0xffffffffull];
    }
    const int32_t i = pfrow[e], col = pcol[e];
    const int32_t J = col / RBM_NCOL, q = col - J * RBM_NCOL, node = i / NS;
    const double own = qt[(int64_t)q * nf + (int64_t)pos[node] * NS + (i - node * NS)];
    const double pt = agg[node] == J ? own : 0.0;
    pval[e] = pt - (omega * s) / diag[i];
  }
}

// the node graph of a coarse level: node I's row is the six scalar rows 6 I .. 6 I + 5 on end, its columns their nodes
__global__ __launch_bounds__(VB) void k_srbm_node_rows(int64_t nn, const rp_t* __restrict__ rowptr, rp_t* __restrict__ noderow)
{
  SAGG_FOR(I, nn + 1)
    noderow[I] = rowptr[I * RBM_NCOL];
}
__global__ __launch_bounds__(VB) void k_srbm_node_cols(int64_t nnz, const int32_t* __restrict__ cols, int32_t* __restrict__ nodecol)
{
  SAGG_FOR(k, nnz)
    nodecol[k] = cols[k] / RBM_NCOL;
}

// the unit diagonal of every dropped coarse dof as one more term of A_c
__global__ __launch_bounds__(VB) void k_srbm_unit_terms(int64_t n, const int32_t* __restrict__ dofs, u64 unit, u64* __restrict__ key,
                                                        u64* __restrict__ val)
{
  SAGG_FOR(t, n)
  {
    const u64 d = (u64)(unsigned)dofs[t];
    key[t] = (d << 32) | d;
    val[t] = unit;
  }
}
static void srbm_write_unit_terms(hipStream_t s, int64_t n, const int32_t* dofs, u64 unit, u64* key, u64* val)
{
  hipLaunchKernelGGL(k_srbm_unit_terms, dim3(grid_cap(n, VB, 1 << 16)), dim3(VB), 0, s, n, dofs, unit, key, val);
}

int64_t srbm_dropped(const SaggLevel* S) { return S->ndrop; }
const double* srbm_nns(const SaggLevel* S, bool coarse) { return coarse ? S->Bc.p : S->B.p; }

// The aggregates of level f: ZZZ_PC_AGG's rule on its node graph
int srbm_aggregate(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, int level)
{
  if (!S->agg)
    S->agg = agg_new();
  S->tag = "-pc_type sagg_rbm";
  S->ns = level == 0 ? 3 : RBM_NCOL;
  if (level == 0)
    return agg_aggregate(ctx, f, S->agg); // (block size 3: the context's own node graph)
  hipStream_t s = ctx->stream;
  const int64_t nn = f->n_owned / RBM_NCOL, N = f->nnz;
  DevBuf<rp_t> noderow;
  DevBuf<int32_t> nodecol;
  DevBuf<uint8_t> free_;
  ZZZ_HIP(ctx, noderow.alloc((size_t)nn + 1));
  ZZZ_HIP(ctx, nodecol.alloc((size_t)N));
  ZZZ_HIP(ctx, free_.alloc((size_t)nn));
  ZZZ_HIP(ctx, hipMemsetAsync(free_.p, 0, (size_t)nn, s)); // (a coarse level has no constrained dofs)
  hipLaunchKernelGGL(k_srbm_node_rows, dim3(grid_cap(nn + 1, VB, 1 << 16)), dim3(VB), 0, s, nn, f->rowptr.p, noderow.p);
  hipLaunchKernelGGL(k_srbm_node_cols, dim3(grid_cap(N, VB, 1 << 16)), dim3(VB), 0, s, N, f->cols.p, nodecol.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return agg_aggregate_graph(ctx, nn, N, noderow.p, nodecol.p, f->vals.p, free_.p, S->agg); // (ends synchronised: the three are locals)
}

// B of the level, the orthogonalisation, and P's pattern and term list
template <int NS>
static int srbm_structure_ns(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, const SaggLevel* above, double omega, zzz_ctx* c, int level,
                             int* max_row)
{
  const bool rows = ctx->mg_products == ZZZ_MG_PRODUCTS_ROWS; // (zzz_sagg_rows.hip: no term positions, so no limit on them)
  hipStream_t s = ctx->stream;
  const int64_t N = f->nnz, nf = f->n_owned * f->bs, nn = nf / NS, nagg = agg_count(S.agg), nc = nagg * RBM_NCOL;
  S.bs = f->bs;
  S.nf = nf;
  S.nc = nc;
  if (!rows && (uint64_t)nf * RBM_NCOL >= (1ull << 32))
    return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: %lld dofs: 32-bit term positions take six values per dof", S.tag, level, (long long)nf);
  SaggFrame Fr;
  if (rows)
    Fr.perm = f->dofmap.renumbered ? f->perm.p : nullptr;
  else if (int rc = sagg_frame(ctx, f, Fr))
    return rc;
  const int32_t* agg = agg_map(S.agg);
  const int g = grid_cap(N, VB, 1 << 16), gf = grid_cap(nf, VB, 1 << 16);
  // ---- B, the rows of the aggregates, Q and R ---------------------------------------------------
  const double* B = above ? above->Bc.p : nullptr;
  if (!above)
  {
    ZZZ_HIP(ctx, S.B.alloc((size_t)(RBM_NCOL * nf)));
    hipLaunchKernelGGL(k_srbm_b0, dim3(gf), dim3(VB), 0, s, nf, f->dofmap.near_null_ld, f->near_null.p, f->bc.p, Fr.perm, S.B.p);
    B = S.B.p;
  }
  DevBuf<int32_t> dscan;
  ZZZ_HIP(ctx, S.qt.alloc((size_t)(RBM_NCOL * nf)));
  ZZZ_HIP(ctx, S.pos.alloc((size_t)nn));
  ZZZ_HIP(ctx, S.Bc.alloc((size_t)(RBM_NCOL * nc)));
  ZZZ_HIP(ctx, S.drop.alloc((size_t)nc + 1));
  ZZZ_HIP(ctx, dscan.alloc((size_t)nc + 1));
  ZZZ_HIP(ctx, hipMemsetAsync(S.drop.p + nc, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_srbm_member_pos, dim3(grid_cap(nn, VB, 1 << 16)), dim3(VB), 0, s, nn, agg_members(S.agg), S.pos.p);
  hipLaunchKernelGGL(k_srbm_gather_rows<NS>, dim3(gf), dim3(VB), 0, s, nf, agg_members(S.agg), f->bc.p, Fr.perm, B, S.qt.p);
  hipLaunchKernelGGL(k_srbm_qr, dim3(grid_cap(nagg, VB / 64, 1 << 20)), dim3(VB), 0, s, nagg, NS, nf, nc, agg_member_offsets(S.agg), S.qt.p,
                     S.Bc.p, S.drop.p);
  if (int rc = with_scratch(ctx, Fr.W.tmp, scan_excl(S.drop.p, dscan.p, (size_t)nc + 1, s)))
    return rc;
  int32_t nd = 0;
  ZZZ_HIP(ctx, dev_fetch(ctx, dscan.p + nc, &nd));
  S.ndrop = nd;
  ZZZ_HIP(ctx, S.droplist.alloc((size_t)nd));
  if (nd > 0)
    hipLaunchKernelGGL(k_srbm_drop_list, dim3(grid_cap(nc, VB, 1 << 16)), dim3(VB), 0, s, nc, S.drop.p, dscan.p, S.droplist.p);
  if (rows)
  {
    ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (dscan is a local)
    return sagg_rows_build(ctx, f, S, SaggPt::RBM, omega, c, level, max_row); // (P, R, T and A_c with their values)
  }
  // ---- P ------------------------------------------------------------------------------------
  hipLaunchKernelGGL(k_srbm_p_count<NS>, dim3(g), dim3(VB), 0, s, N, Fr.order, Fr.rowidx.p, f->cols.p, f->bc.p, agg, S.drop.p, Fr.W.cnt.p);
  int64_t pterms = 0;
  if (int rc = sagg_term_offsets(ctx, S, Fr.W, N, level, "A P_t", 0, &pterms))
    return rc;
  if (pterms <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: the prolongator to %lld coarse dofs is empty", S.tag, level, (long long)nc);
  hipLaunchKernelGGL(k_srbm_p_terms<NS>, dim3(g), dim3(VB), 0, s, N, nf, Fr.order, Fr.rowidx.p, f->cols.p, f->bc.p, agg, S.drop.p, S.pos.p,
                       Fr.W.off.p, Fr.W.k0.p, Fr.W.v0.p);
  ZZZ_HIP(ctx, hipGetLastError());
  if (int rc = sagg_p_from_terms(ctx, S, Fr, pterms, level))
    return rc;
  SaggUnitTerms unit;
  unit.n = nd;
  unit.dofs = S.droplist.p;
  unit.write = srbm_write_unit_terms;
  return sagg_products(ctx, f, S, c, level, Fr, unit, max_row); // (ends synchronised: dscan is a local)
}

// the values of P from f's matrix values and qt, then R's, T's and A_c's
static int srbm_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, double omega, zzz_ctx* c)
{
  hipStream_t s = ctx->stream;
  const int gp = grid_cap(S.pnnz, VB, 1 << 16);
  const int32_t* agg = agg_map(S.agg);
  sagg_diagonal(ctx, f, S);
  if (S.ns == 3)
    hipLaunchKernelGGL(k_srbm_p_values<3>, dim3(gp), dim3(VB), 0, s, S.pnnz, S.nf, S.pseg.p, S.psrc.p, f->vals.p, S.qt.p, S.pfrow.p, S.pcol.p,
                       agg, S.pos.p, S.diag.p, omega, S.pval.p);
  else
    hipLaunchKernelGGL(k_srbm_p_values<RBM_NCOL>, dim3(gp), dim3(VB), 0, s, S.pnnz, S.nf, S.pseg.p, S.psrc.p, f->vals.p, S.qt.p, S.pfrow.p,
                       S.pcol.p, agg, S.pos.p, S.diag.p, omega, S.pval.p);
  return sagg_product_values(ctx, f, S, c);
}

// above: the level above f (null: f is level 0, whose B is the context's near-nullspace)
int srbm_galerkin(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, const SaggLevel* above, double omega, zzz_ctx* c, int level)
{
  int max_row = 0;
  if (int rc = S->ns == 3 ? srbm_structure_ns<3>(ctx, f, *S, above, omega, c, level, &max_row)
                          : srbm_structure_ns<RBM_NCOL>(ctx, f, *S, above, omega, c, level, &max_row))
    return rc;
  if (!S->rows)
    if (int rc = srbm_values(ctx, f, *S, omega, c))
      return rc;
  if (int rc = ctx_adopt_csr(c, 1, S->nc, S->cnnz, max_row)) // (scalar: the node size is the level's)
    return fail(ctx, rc, "%s: the coarse level of %lld dofs: %s", S->tag, (long long)S->nc, c->err.c_str());
  return ZZZ_OK;
}

int srbm_refresh(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c)
{
  if (int rc = S->rows ? sagg_rows_values(ctx, f, *S, SaggPt::RBM, omega, c) : srbm_values(ctx, f, *S, omega, c))
    return rc;
  return ctx_adopt_values(c);
}
ZZZ_PRELOAD_TU(sagg_rbm)
} // namespace zzz
