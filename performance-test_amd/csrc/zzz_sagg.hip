// ZZZ_PC_SAGG: smoothed-aggregation multigrid from the assembled matrix alone (PETSc's -pc_type gamg -pc_gamg_agg_nsmooths 1
// without a near-nullspace): ZZZ_PC_AGG (zzz_agg.hip) with one prolongator-smoothing step.  This file holds what the step
// adds: the stored prolongator P and its transpose, the two products A P and P^T (A P), and the two transfer kernels.  The
// aggregates are zzz_agg.hip's; levels, smoother, V-cycle, dense coarsest solve, caching and profiling are zzz_mg.hip's.
//
// The rule, per level (tests/_sagg_ref.py restates it sum for sum).  Every sum is a chain of plain double additions of
// individually rounded products (no fused multiply-add), in ASCENDING index: of the caller's numbering on level 0, of the
// level's own numbering below.
//   aggregates  ZZZ_PC_AGG's rule (agg_aggregate) on the graph of this level's matrix.
//   P_t         ZZZ_PC_AGG's P: 1 from each unconstrained scalar dof (i, c) to (aggregate(i), c).
//   omega       4 / (3 hi), hi the bound of D^-1 A that this level's smoother uses (min(Gershgorin, 1.1 x Lanczos estimate),
//               pc_esteig_its): a level's bound comes before the next level's values.
//   P           (I - omega D^-1 A) P_t, CSR with ascending coarse columns.  Pattern: (i, J) wherever row i is unconstrained
//               and has a structural entry a_ik, zero or not, with k unconstrained and mapped to J by P_t.  Value:
//               s = sum_k a_ik over those k;  P(i, J) = delta - (omega s) / a_ii,  delta = 1 when P_t(i, J) = 1, else 0.
//               Rows of constrained dofs are empty.
//   R           P^T as CSR, coarse rows with ascending fine index: the restriction is a gather, summed in one fixed order
//               (a wavefront per coarse row: lane l adds the entries l, l + 64, ... front to back, the 64 sums meet in the
//               shuffle tree, as in zzz_mg.hip's dense solve).
//   T           A P:  T(i, J) = sum_k a_ik P(k, J).
//   A_c         P^T T:  A_c(I, J) = sum_i P(i, I) T(i, J); its pattern is every (I, J) that receives a structural term.  The
//               child context adopts it as ZZZ_PC_AGG's: block size kept, no Dirichlet rows.
// Each of P, T and A_c is formed the way agg_galerkin_bs forms its sum: the terms are written out in ascending order of the
// summation index with a 64-bit (row, column) key, a STABLE radix sort (rocPRIM) brings equal keys together in that order,
// and one thread sums each run front to back.  The sorted term lists are kept: a refresh is the sums alone, and gives the
// bits of a fresh set-up.  Term positions are 32-bit: a level with more terms is refused (ZZZ_ERR_LIMIT), never wrapped.
//
// ZZZ_PC_SAGG_RBM (zzz_sagg_rbm.hip) differs in P's terms and P's value kernel alone: the level (SaggLevel) and the host steps
// from P's terms on -- sagg_p_from_terms, sagg_products, sagg_product_values, the transfers -- are declared in zzz_sagg.h and
// serve both.  Its dropped coarse dofs reach A_c as one more term each (SaggUnitTerms).
//
// zzz_mg_products(ZZZ_MG_PRODUCTS_ROWS) forms the same products row by row, with no term list (zzz_sagg_rows.hip): sagg_galerkin
// and sagg_refresh branch on it here, R is built by sagg_transpose_p in both modes, and the transfers read the same arrays.
#include "zzz_sagg.h"

#include <cstdlib>
#include <vector>

namespace zzz
{
constexpr int64_t SAGG_MAX_TERMS = (int64_t)INT32_MAX - 16;

// the scalar row of every matrix entry
__global__ __launch_bounds__(VB) void k_sagg_rowidx(int64_t nrows, const rp_t* __restrict__ rowptr, int32_t* __restrict__ rowidx)
{
  SAGG_FOR(r, nrows)
    for (rp_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
      rowidx[k] = (int32_t)r;
}

// level 0 in an internal order: the entries' (row, column) in the caller's numbering, to be sorted first
template <int BS>
__global__ __launch_bounds__(VB) void k_sagg_caller_keys(int64_t nnz, const int32_t* __restrict__ rowidx, const int32_t* __restrict__ cols,
                                                         const int32_t* __restrict__ perm, u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(k, nnz)
  {
    key[k] = (sagg_caller<BS>(perm, rowidx[k]) << 32) | sagg_caller<BS>(perm, cols[k]);
    val[k] = (u64)k;
  }
}

// P's terms: matrix entry k = order[t] (order null: t) of an unconstrained row and column goes to (row, coarse dof of the column)
template <int BS>
__global__ __launch_bounds__(VB) void k_sagg_p_keys(int64_t nnz, const u64* __restrict__ order, const int32_t* __restrict__ rowidx,
                                                    const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                    const int32_t* __restrict__ agg, u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(t, nnz)
  {
    const int32_t k = order ? (int32_t)order[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    const int32_t J = agg[c / BS];
    const bool ok = J >= 0 && bc[r] == 0 && bc[c] == 0;
    key[t] = ok ? (((u64)r << 32) | ((u64)(J >= 0 ? J : 0) * BS + (unsigned)(c % BS))) : SAGG_NOKEY;
    val[t] = (u64)k << 32;
  }
}

// head[t] = sorted term t opens a run
__global__ __launch_bounds__(VB) void k_sagg_heads(int64_t n, const u64* __restrict__ key, int32_t* __restrict__ head)
{
  SAGG_FOR(t, n)
  {
    const u64 a = key[t > 0 ? t - 1 : 0], b = key[t];
    head[t] = (b != SAGG_NOKEY && (t == 0 || a != b)) ? 1 : 0;
    if (t == 0)
      head[n] = 0;
  }
}

// run e = pos[t] of every head t: where it starts, its column, its row; the end of the last run
__global__ __launch_bounds__(VB) void k_sagg_entries(int64_t n, int64_t nruns, const u64* __restrict__ key, const int32_t* __restrict__ head,
                                                     const int32_t* __restrict__ pos, int32_t* __restrict__ seg, int32_t* __restrict__ ecol,
                                                     int32_t* __restrict__ erow)
{
  SAGG_FOR(t, n)
  {
    const u64 b = key[t], nx = key[t + 1 < n ? t + 1 : t];
    const int32_t h = head[t], e = pos[t];
    if (h)
    {
      seg[e] = (int32_t)t;
      ecol[e] = (int32_t)(b & 0xffffffffull);
      erow[e] = (int32_t)(b >> 32);
    }
    if (b != SAGG_NOKEY && (t + 1 == n || nx == SAGG_NOKEY))
      seg[nruns] = (int32_t)(t + 1);
  }
}

// off[a] = first position of row a in the ascending rows (a = 0 .. nrows)
__global__ __launch_bounds__(VB) void k_sagg_offsets(const int32_t* __restrict__ rows, int64_t n, int64_t nrows, rp_t* __restrict__ off)
{
  SAGG_FOR(t, n + 1)
  {
    const int64_t a = rows[t > 0 ? t - 1 : 0], b = rows[t < n ? t : n - 1];
    const int64_t lo = t == 0 ? -1 : (a < nrows ? a : nrows);
    const int64_t hi = t == n ? nrows : (b < nrows ? b : nrows);
    for (int64_t s = lo + 1; s <= hi; ++s)
      off[s] = (rp_t)t;
  }
}

// R's sort input: P's entry e under (coarse column, fine row in the caller's numbering)
template <int BS>
__global__ __launch_bounds__(VB) void k_sagg_r_keys(int64_t pnnz, const int32_t* __restrict__ pfrow, const int32_t* __restrict__ pcol,
                                                    const int32_t* __restrict__ perm, u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(e, pnnz)
  {
    key[e] = ((u64)pcol[e] << 32) | sagg_caller<BS>(perm, pfrow[e]);
    val[e] = (u64)e;
  }
}
// ... and R's entries from the sorted pairs
__global__ __launch_bounds__(VB) void k_sagg_r_entries(int64_t pnnz, const u64* __restrict__ key, const u64* __restrict__ src,
                                                       const int32_t* __restrict__ pfrow, int32_t* __restrict__ rsrc,
                                                       int32_t* __restrict__ rfine, int32_t* __restrict__ rcrow)
{
  SAGG_FOR(t, pnnz)
  {
    const int32_t e = (int32_t)src[t];
    rsrc[t] = e;
    rfine[t] = pfrow[e];
    rcrow[t] = (int32_t)(key[t] >> 32);
  }
}

// terms of T that matrix entry order[t] brings: the entries of P's row of its column (none in a constrained row)
__global__ __launch_bounds__(VB) void k_sagg_t_count(int64_t nnz, const u64* __restrict__ order, const int32_t* __restrict__ rowidx,
                                                     const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                     const rp_t* __restrict__ prow, int32_t* __restrict__ cnt)
{
  SAGG_FOR(t, nnz)
  {
    const int32_t k = order ? (int32_t)order[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    const int32_t len = (int32_t)(prow[c + 1] - prow[c]);
    cnt[t] = bc[r] == 0 ? len : 0;
    if (t == 0)
      cnt[nnz] = 0;
  }
}
// ... written out: key (row in the caller's numbering, coarse column), value (matrix entry, entry of P)
template <int BS>
__global__ __launch_bounds__(VB) void k_sagg_t_terms(int64_t nnz, const u64* __restrict__ order, const int32_t* __restrict__ rowidx,
                                                     const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                     const int32_t* __restrict__ perm, const rp_t* __restrict__ prow,
                                                     const int32_t* __restrict__ pcol, const int64_t* __restrict__ off,
                                                     u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(t, nnz)
  {
    const int32_t k = order ? (int32_t)order[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    if (bc[r] != 0)
      continue;
    const u64 R = sagg_caller<BS>(perm, r) << 32;
    const rp_t q0 = prow[c], q1 = prow[c + 1];
    const int64_t o = off[t];
    for (rp_t q = q0; q < q1; ++q)
    {
      key[o + (q - q0)] = R | (u64)(unsigned)pcol[q];
      val[o + (q - q0)] = ((u64)k << 32) | (u64)q;
    }
  }
}
// the stored row of every entry of T: that of the first matrix entry of its run
__global__ __launch_bounds__(VB) void k_sagg_t_rows(int64_t tnnz, const int32_t* __restrict__ tseg, const u64* __restrict__ tsrc,
                                                    const int32_t* __restrict__ rowidx, int32_t* __restrict__ tfrow)
{
  SAGG_FOR(e, tnnz)
    tfrow[e] = rowidx[tsrc[tseg[e]] >> 32];
}

// terms of A_c that entry e of T brings: the entries of P's row of its row
__global__ __launch_bounds__(VB) void k_sagg_c_count(int64_t tnnz, const int32_t* __restrict__ tfrow, const rp_t* __restrict__ prow,
                                                     int32_t* __restrict__ cnt)
{
  SAGG_FOR(e, tnnz)
  {
    const int32_t i = tfrow[e];
    cnt[e] = (int32_t)(prow[i + 1] - prow[i]);
    if (e == 0)
      cnt[tnnz] = 0;
  }
}
// ... written out: key (coarse row, coarse column), value (entry of T, entry of P)
__global__ __launch_bounds__(VB) void k_sagg_c_terms(int64_t tnnz, const int32_t* __restrict__ tfrow, const int32_t* __restrict__ tcol,
                                                     const rp_t* __restrict__ prow, const int32_t* __restrict__ pcol,
                                                     const int64_t* __restrict__ off, u64* __restrict__ key, u64* __restrict__ val)
{
  SAGG_FOR(e, tnnz)
  {
    const int32_t i = tfrow[e];
    const u64 J = (u64)(unsigned)tcol[e];
    const rp_t q0 = prow[i], q1 = prow[i + 1];
    const int64_t o = off[e];
    for (rp_t q = q0; q < q1; ++q)
    {
      key[o + (q - q0)] = ((u64)(unsigned)pcol[q] << 32) | J;
      val[o + (q - q0)] = ((u64)e << 32) | (u64)q;
    }
  }
}

// a_ii of every row (0 where the pattern has no diagonal entry)
__global__ __launch_bounds__(VB) void k_sagg_diag(int64_t nrows, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                  const double* __restrict__ vals, double* __restrict__ diag)
{
  SAGG_FOR(r, nrows)
  {
    double d = 0.0;
    for (rp_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
    {
      const int32_t c = cols[k];
      const double v = vals[k];
      d = c == (int32_t)r ? v : d;
    }
    diag[r] = d;
  }
}

// P(i, J) = delta - (omega s) / a_ii, s the run's matrix entries summed front to back
template <int BS>
__global__ __launch_bounds__(VB) void k_sagg_p_values(int64_t pnnz, const int32_t* __restrict__ pseg, const u64* __restrict__ psrc,
                                                      const double* __restrict__ a, const int32_t* __restrict__ pfrow,
                                                      const int32_t* __restrict__ pcol, const int32_t* __restrict__ agg,
                                                      const double* __restrict__ diag, double omega, double* __restrict__ pval)
{
  SAGG_FOR(e, pnnz)
  {
    double s = 0.0;
    for (int32_t t = pseg[e]; t < pseg[e + 1]; ++t)
      s += a[psrc[t] >> 32];
    const int32_t i = pfrow[e];
    const double delta = pcol[e] == agg[i / BS] * BS + i % BS ? 1.0 : 0.0;
    pval[e] = delta - (omega * s) / diag[i];
  }
}

__global__ __launch_bounds__(VB) void k_sagg_gather(int64_t n, const int32_t* __restrict__ src, const double* __restrict__ in,
                                                    double* __restrict__ out)
{
  SAGG_FOR(t, n)
    out[t] = in[src[t]];
}

// out[e] = sum over the run of e of hi[src >> 32] * lo[src & 0xffffffff], front to back
__global__ __launch_bounds__(VB) void k_sagg_sum_products(int64_t n, const int32_t* __restrict__ seg, const u64* __restrict__ src,
                                                          const double* __restrict__ hi, const double* __restrict__ lo,
                                                          double* __restrict__ out)
{
  SAGG_FOR(e, n)
  {
    double s = 0.0;
    for (int32_t t = seg[e]; t < seg[e + 1]; ++t)
    {
      const u64 p = src[t];
      s += hi[p >> 32] * lo[p & 0xffffffffull];
    }
    out[e] = s;
  }
}

// out[0] = the longest coarse row (an integer maximum), out[1] = the empty ones (an integer sum)
__global__ __launch_bounds__(VB) void k_sagg_rowstats(int64_t nrows, const rp_t* __restrict__ rowptr, int32_t* __restrict__ out)
{
  SAGG_FOR(r, nrows)
  {
    const int32_t len = (int32_t)(rowptr[r + 1] - rowptr[r]);
    atomicMax(&out[0], len);
    if (len == 0)
      atomicAdd(&out[1], 1);
  }
}

// r_c = R (r_f - sub): a wavefront per coarse dof (a row of R holds tens to hundreds of entries: the fine dofs of an aggregate
// and of its neighbours), entries and values read coalesced; lane l adds the entries l, l + 64, ... front to back and the 64
// sums meet in the shuffle tree -- one fixed order, no atomics, the same bits in every run.  (Constrained fine dofs have no
// entry in R.)
__global__ __launch_bounds__(VB) void k_sagg_restrict(const int* __restrict__ stop, int64_t nc, const rp_t* __restrict__ rrow,
                                                      const int32_t* __restrict__ rfine, const double* __restrict__ rval,
                                                      const double* __restrict__ rf, const double* __restrict__ sub,
                                                      double* __restrict__ rc)
{
  if (stop && *stop)
    return;
  const int lane = threadIdx.x & 63;
  for (int64_t J = blockIdx.x * (int64_t)(VB / 64) + (threadIdx.x >> 6); J < nc; J += (int64_t)gridDim.x * (VB / 64))
  {
    double acc = 0.0;
    for (rp_t t = rrow[J] + lane; t < rrow[J + 1]; t += 64)
    {
      const int32_t i = rfine[t];
      const double w = rval[t];
      const double v = sub ? rf[i] - sub[i] : rf[i];
      acc += w * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      acc += __shfl_down(acc, o, 64);
    if (lane == 0)
      rc[J] = acc;
  }
}

// x_f (+)= P e_c: a thread per fine dof sums its row of P front to back (an empty row: zero)
__global__ __launch_bounds__(VB) void k_sagg_prolong(const int* __restrict__ stop, int64_t nf, const rp_t* __restrict__ prow,
                                                     const int32_t* __restrict__ pcol, const double* __restrict__ pval,
                                                     const double* __restrict__ ec, double* __restrict__ xf, int accumulate)
{
  if (stop && *stop)
    return;
  SAGG_FOR(d, nf)
  {
    double s = 0.0;
    for (rp_t q = prow[d]; q < prow[d + 1]; ++q)
    {
      const double w = pval[q];
      const double e = ec[pcol[q]];
      s += w * e;
    }
    xf[d] = accumulate ? xf[d] + s : s;
  }
}

SaggLevel* sagg_new() { return new SaggLevel(); }
void sagg_free(SaggLevel* S) { delete S; }
int64_t sagg_count(const SaggLevel* S) { return S->agg ? agg_count(S->agg) : 0; }
int64_t sagg_p_nnz(const SaggLevel* S) { return S->pnnz; }

int sagg_aggregate(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S)
{
  if (!S->agg)
    S->agg = agg_new();
  return agg_aggregate(ctx, f, S->agg);
}

// the most terms one product of a level may have (ZZZ_SAGG_MAX_TERMS lowers it: the refusal at a size a test can reach)
static int64_t sagg_term_limit()
{
  const char* e = getenv("ZZZ_SAGG_MAX_TERMS");
  const long long v = e ? atoll(e) : 0;
  return v > 0 && v < SAGG_MAX_TERMS ? (int64_t)v : SAGG_MAX_TERMS;
}

// n terms in W.k0 / W.v0 -> the keys sorted into W.k1, the values beside them into src, heads and positions of the runs of
// equal keys (SAGG_NOKEY belongs to none); *nruns = how many
static int sagg_sort_runs(zzz_ctx* ctx, SaggWork& W, int64_t n, DevBuf<u64>& src, int64_t* nruns)
{
  hipStream_t s = ctx->stream;
  ZZZ_HIP(ctx, W.k1.alloc((size_t)n));
  ZZZ_HIP(ctx, src.alloc((size_t)n));
  ZZZ_HIP(ctx, W.head.alloc((size_t)n + 1));
  ZZZ_HIP(ctx, W.pos.alloc((size_t)n + 1));
  if (int rc = with_scratch(ctx, W.tmp, sort_pairs(W.k0.p, W.k1.p, W.v0.p, src.p, (size_t)n, 0, 64, s)))
    return rc;
  hipLaunchKernelGGL(k_sagg_heads, dim3(grid_cap(n, VB, 1 << 16)), dim3(VB), 0, s, n, W.k1.p, W.head.p);
  if (int rc = with_scratch(ctx, W.tmp, scan_excl(W.head.p, W.pos.p, (size_t)n + 1, s)))
    return rc;
  int32_t r = 0;
  ZZZ_HIP(ctx, dev_fetch(ctx, W.pos.p + n, &r));
  *nruns = r;
  return ZZZ_OK;
}

int sagg_term_offsets(zzz_ctx* ctx, const SaggLevel& S, SaggWork& W, int64_t n, int level, const char* what, int64_t extra,
                      int64_t* total)
{
  ZZZ_HIP(ctx, W.off.alloc((size_t)n + 1));
  if (int rc = with_scratch(ctx, W.tmp, scan_excl(W.cnt.p, W.off.p, (size_t)n + 1, ctx->stream)))
    return rc;
  ZZZ_HIP(ctx, dev_fetch(ctx, W.off.p + n, total));
  const int64_t limit = sagg_term_limit();
  if (*total + extra > limit)
    return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: %lld terms of %s, 32-bit term positions take %lld", S.tag, level,
                (long long)(*total + extra), what, (long long)limit);
  ZZZ_HIP(ctx, W.k0.alloc((size_t)(*total + extra)));
  ZZZ_HIP(ctx, W.v0.alloc((size_t)(*total + extra)));
  return ZZZ_OK;
}

template <int BS>
static int sagg_frame_bs(zzz_ctx* ctx, zzz_ctx* f, SaggFrame& Fr)
{
  hipStream_t s = ctx->stream;
  const int64_t N = f->nnz, nf = f->n_owned * BS;
  SaggWork& W = Fr.W;
  Fr.perm = f->dofmap.renumbered ? f->perm.p : nullptr;
  ZZZ_HIP(ctx, Fr.rowidx.alloc((size_t)N));
  ZZZ_HIP(ctx, W.k0.alloc((size_t)N));
  ZZZ_HIP(ctx, W.v0.alloc((size_t)N));
  ZZZ_HIP(ctx, W.cnt.alloc((size_t)N + 1));
  hipLaunchKernelGGL(k_sagg_rowidx, dim3(grid_cap(nf, VB, 1 << 16)), dim3(VB), 0, s, nf, f->rowptr.p, Fr.rowidx.p);
  Fr.order = nullptr;
  if (Fr.perm)
  {
    ZZZ_HIP(ctx, W.k1.alloc((size_t)N));
    ZZZ_HIP(ctx, Fr.ordbuf.alloc((size_t)N));
    hipLaunchKernelGGL(k_sagg_caller_keys<BS>, dim3(grid_cap(N, VB, 1 << 16)), dim3(VB), 0, s, N, Fr.rowidx.p, f->cols.p, Fr.perm, W.k0.p, W.v0.p);
    if (int rc = with_scratch(ctx, W.tmp, sort_pairs(W.k0.p, W.k1.p, W.v0.p, Fr.ordbuf.p, (size_t)N, 0, 64, s)))
      return rc;
    Fr.order = Fr.ordbuf.p;
  }
  return ZZZ_OK;
}
int sagg_frame(zzz_ctx* ctx, zzz_ctx* f, SaggFrame& Fr)
{
  return f->bs == 3 ? sagg_frame_bs<3>(ctx, f, Fr) : sagg_frame_bs<1>(ctx, f, Fr);
}

int sagg_p_from_terms(zzz_ctx* ctx, SaggLevel& S, SaggFrame& Fr, int64_t n, int level)
{
  hipStream_t s = ctx->stream;
  SaggWork& W = Fr.W;
  S.pterms = n;
  if (int rc = sagg_sort_runs(ctx, W, n, S.psrc, &S.pnnz))
    return rc;
  if (S.pnnz <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: the prolongator to %lld coarse dofs is empty", S.tag, level, (long long)S.nc);
  const int gp = grid_cap(S.pnnz, VB, 1 << 16);
  ZZZ_HIP(ctx, S.pseg.alloc((size_t)S.pnnz + 1));
  ZZZ_HIP(ctx, S.pcol.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, S.pfrow.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, S.pval.alloc((size_t)S.pnnz + 1));
  ZZZ_HIP(ctx, S.diag.alloc((size_t)S.nf));
  ZZZ_HIP(ctx, S.prow.alloc((size_t)S.nf + 1));
  hipLaunchKernelGGL(k_sagg_entries, dim3(grid_cap(n, VB, 1 << 16)), dim3(VB), 0, s, n, S.pnnz, W.k1.p, W.head.p, W.pos.p, S.pseg.p, S.pcol.p,
                     S.pfrow.p);
  hipLaunchKernelGGL(k_sagg_offsets, dim3(gp), dim3(VB), 0, s, S.pfrow.p, S.pnnz, S.nf, S.prow.p);
  return ZZZ_OK;
}

// ---- R: P's entries under (coarse column, fine row in the caller's numbering); the keys are distinct ----------
template <int BS>
static int sagg_transpose_p_bs(zzz_ctx* ctx, SaggLevel& S, const int32_t* perm, const int32_t* pfrow, SaggWork& W)
{
  hipStream_t s = ctx->stream;
  const int gp = grid_cap(S.pnnz, VB, 1 << 16);
  DevBuf<int32_t> erow;
  DevBuf<u64> rtmp;
  ZZZ_HIP(ctx, S.rrow.alloc((size_t)S.nc + 1));
  ZZZ_HIP(ctx, S.rfine.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, S.rsrc.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, S.rval.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, erow.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, rtmp.alloc((size_t)S.pnnz));
  ZZZ_HIP(ctx, W.k0.reserve((size_t)S.pnnz)); // (the lists mode: they hold P's terms, which are at least as many)
  ZZZ_HIP(ctx, W.v0.reserve((size_t)S.pnnz));
  ZZZ_HIP(ctx, W.k1.reserve((size_t)S.pnnz));
  hipLaunchKernelGGL(k_sagg_r_keys<BS>, dim3(gp), dim3(VB), 0, s, S.pnnz, pfrow, S.pcol.p, perm, W.k0.p, W.v0.p);
  if (int rc = with_scratch(ctx, W.tmp, sort_pairs(W.k0.p, W.k1.p, W.v0.p, rtmp.p, (size_t)S.pnnz, 0, 64, s)))
    return rc;
  hipLaunchKernelGGL(k_sagg_r_entries, dim3(gp), dim3(VB), 0, s, S.pnnz, W.k1.p, rtmp.p, pfrow, S.rsrc.p, S.rfine.p, erow.p);
  hipLaunchKernelGGL(k_sagg_offsets, dim3(gp), dim3(VB), 0, s, erow.p, S.pnnz, S.nc, S.rrow.p);
  ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (erow and rtmp are locals)
  return ZZZ_OK;
}
int sagg_transpose_p(zzz_ctx* ctx, SaggLevel& S, const int32_t* perm, const int32_t* pfrow, SaggWork& W)
{
  return S.bs == 3 ? sagg_transpose_p_bs<3>(ctx, S, perm, pfrow, W) : sagg_transpose_p_bs<1>(ctx, S, perm, pfrow, W);
}
void sagg_row_index(zzz_ctx* ctx, int64_t nrows, const rp_t* rowptr, int32_t* rowidx)
{
  hipLaunchKernelGGL(k_sagg_rowidx, dim3(grid_cap(nrows, VB, 1 << 16)), dim3(VB), 0, ctx->stream, nrows, rowptr, rowidx);
}
void sagg_r_values(zzz_ctx* ctx, SaggLevel& S)
{
  hipLaunchKernelGGL(k_sagg_gather, dim3(grid_cap(S.pnnz, VB, 1 << 16)), dim3(VB), 0, ctx->stream, S.pnnz, S.rsrc.p, S.pval.p, S.rval.p);
}
void sagg_row_stats(zzz_ctx* ctx, int64_t nrows, const rp_t* rowptr, int32_t* out)
{
  hipLaunchKernelGGL(k_sagg_rowstats, dim3(grid_cap(nrows, VB, 1 << 16)), dim3(VB), 0, ctx->stream, nrows, rowptr, out);
}

template <int BS>
static int sagg_products_bs(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c, int level, SaggFrame& Fr, const SaggUnitTerms& unit,
                            int* max_row)
{
  hipStream_t s = ctx->stream;
  const int64_t N = f->nnz, nc = S.nc;
  const int32_t* perm = Fr.perm;
  const u64* order = Fr.order;
  const int32_t* rowidx = Fr.rowidx.p;
  const int g = grid_cap(N, VB, 1 << 16);
  SaggWork& W = Fr.W;
  DevBuf<int32_t> erow, tcol, tfrow, stats;
  ZZZ_HIP(ctx, stats.alloc(2));
  if (int rc = sagg_transpose_p(ctx, S, perm, S.pfrow.p, W))
    return rc;
  // ---- T = A P -------------------------------------------------------------------------------
  ZZZ_HIP(ctx, W.cnt.alloc((size_t)N + 1));
  hipLaunchKernelGGL(k_sagg_t_count, dim3(g), dim3(VB), 0, s, N, order, rowidx, f->cols.p, f->bc.p, S.prow.p, W.cnt.p);
  if (int rc = sagg_term_offsets(ctx, S, W, N, level, "A P", 0, &S.tterms))
    return rc;
  hipLaunchKernelGGL(k_sagg_t_terms<BS>, dim3(g), dim3(VB), 0, s, N, order, rowidx, f->cols.p, f->bc.p, perm, S.prow.p, S.pcol.p,
                     W.off.p, W.k0.p, W.v0.p);
  if (int rc = sagg_sort_runs(ctx, W, S.tterms, S.tsrc, &S.tnnz))
    return rc;
  const int gtt = grid_cap(S.tterms, VB, 1 << 16), gt = grid_cap(S.tnnz, VB, 1 << 16);
  ZZZ_HIP(ctx, S.tseg.alloc((size_t)S.tnnz + 1));
  ZZZ_HIP(ctx, S.tval.alloc((size_t)S.tnnz + 1));
  ZZZ_HIP(ctx, tcol.alloc((size_t)S.tnnz));
  ZZZ_HIP(ctx, tfrow.alloc((size_t)S.tnnz));
  ZZZ_HIP(ctx, erow.alloc((size_t)S.tnnz));
  hipLaunchKernelGGL(k_sagg_entries, dim3(gtt), dim3(VB), 0, s, S.tterms, S.tnnz, W.k1.p, W.head.p, W.pos.p, S.tseg.p, tcol.p, erow.p);
  hipLaunchKernelGGL(k_sagg_t_rows, dim3(gt), dim3(VB), 0, s, S.tnnz, S.tseg.p, S.tsrc.p, rowidx, tfrow.p);
  // ---- A_c = P^T T -----------------------------------------------------------------------------
  ZZZ_HIP(ctx, W.cnt.alloc((size_t)S.tnnz + 1));
  hipLaunchKernelGGL(k_sagg_c_count, dim3(gt), dim3(VB), 0, s, S.tnnz, tfrow.p, S.prow.p, W.cnt.p);
  if (int rc = sagg_term_offsets(ctx, S, W, S.tnnz, level, "P^T (A P)", unit.n, &S.cterms))
    return rc;
  hipLaunchKernelGGL(k_sagg_c_terms, dim3(gt), dim3(VB), 0, s, S.tnnz, tfrow.p, tcol.p, S.prow.p, S.pcol.p, W.off.p, W.k0.p, W.v0.p);
  if (unit.n > 0)
  {
    // the unit diagonal of a dropped coarse dof: one term of its own, the product of the two slots behind T's and P's values
    const double one = 1.0;
    ZZZ_HIP(ctx, hipMemcpyAsync(S.tval.p + S.tnnz, &one, sizeof(double), hipMemcpyHostToDevice, s));
    ZZZ_HIP(ctx, hipMemcpyAsync(S.pval.p + S.pnnz, &one, sizeof(double), hipMemcpyHostToDevice, s));
    ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (`one` is a local)
    unit.write(s, unit.n, unit.dofs, ((u64)S.tnnz << 32) | (u64)S.pnnz, W.k0.p + S.cterms, W.v0.p + S.cterms);
    S.cterms += unit.n;
  }
  if (int rc = sagg_sort_runs(ctx, W, S.cterms, S.csrc, &S.cnnz))
    return rc;
  if (S.cnnz <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: the coarse matrix of %lld dofs is empty", S.tag, level, (long long)nc);
  const int gc = grid_cap(S.cnnz, VB, 1 << 16);
  ZZZ_HIP(ctx, S.cseg.alloc((size_t)S.cnnz + 1));
  ZZZ_HIP(ctx, erow.alloc((size_t)S.cnnz));
  ZZZ_HIP(ctx, c->rowptr.alloc((size_t)nc + 1));
  ZZZ_HIP(ctx, c->cols.alloc((size_t)S.cnnz + 8));
  ZZZ_HIP(ctx, c->vals.alloc((size_t)S.cnnz + 8));
  ZZZ_HIP(ctx, hipMemsetAsync(c->cols.p + S.cnnz, 0, 8 * sizeof(int32_t), s));
  ZZZ_HIP(ctx, hipMemsetAsync(c->vals.p + S.cnnz, 0, 8 * sizeof(double), s));
  ZZZ_HIP(ctx, hipMemsetAsync(stats.p, 0, 2 * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_sagg_entries, dim3(grid_cap(S.cterms, VB, 1 << 16)), dim3(VB), 0, s, S.cterms, S.cnnz, W.k1.p, W.head.p, W.pos.p,
                     S.cseg.p, c->cols.p, erow.p);
  hipLaunchKernelGGL(k_sagg_offsets, dim3(gc), dim3(VB), 0, s, erow.p, S.cnnz, nc, c->rowptr.p);
  hipLaunchKernelGGL(k_sagg_rowstats, dim3(grid_cap(nc, VB, 1 << 16)), dim3(VB), 0, s, nc, c->rowptr.p, stats.p);
  int32_t hs[2] = {0, 0};
  ZZZ_HIP(ctx, dev_fetch(ctx, stats.p, hs, 2)); // (waits for the stream: the work buffers go out of scope below)
  ZZZ_HIP(ctx, hipGetLastError());
  if (hs[1] > 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: %d coarse dofs have no unconstrained member (aggregates of partly "
                                  "constrained block dofs): the coarse matrix would be singular", S.tag, level, hs[1]);
  *max_row = hs[0];
  return ZZZ_OK;
}
int sagg_products(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c, int level, SaggFrame& Fr, const SaggUnitTerms& unit, int* max_row)
{
  return f->bs == 3 ? sagg_products_bs<3>(ctx, f, S, c, level, Fr, unit, max_row)
                    : sagg_products_bs<1>(ctx, f, S, c, level, Fr, unit, max_row);
}

// The patterns of P, R, T and A_c from f's pattern, Dirichlet bytes and aggregates, and the sorted term lists behind their
// values; c's rowptr / cols / vals are allocated here (values: sagg_values).  *max_row = the longest row of A_c.
template <int BS>
static int sagg_structure_bs(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c, int level, int* max_row)
{
  const int64_t N = f->nnz;
  S.bs = BS;
  S.nf = f->n_owned * BS;
  S.nc = agg_count(S.agg) * BS;
  SaggFrame Fr;
  if (int rc = sagg_frame(ctx, f, Fr))
    return rc;
  hipLaunchKernelGGL(k_sagg_p_keys<BS>, dim3(grid_cap(N, VB, 1 << 16)), dim3(VB), 0, ctx->stream, N, Fr.order, Fr.rowidx.p, f->cols.p,
                     f->bc.p, agg_map(S.agg), Fr.W.k0.p, Fr.W.v0.p);
  if (int rc = sagg_p_from_terms(ctx, S, Fr, N, level))
    return rc;
  return sagg_products(ctx, f, S, c, level, Fr, SaggUnitTerms(), max_row);
}

int sagg_diagonal(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S)
{
  hipLaunchKernelGGL(k_sagg_diag, dim3(grid_cap(S.nf, VB, 1 << 16)), dim3(VB), 0, ctx->stream, S.nf, f->rowptr.p, f->cols.p, f->vals.p,
                     S.diag.p);
  return ZZZ_OK;
}

int sagg_product_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c)
{
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_sagg_gather, dim3(grid_cap(S.pnnz, VB, 1 << 16)), dim3(VB), 0, s, S.pnnz, S.rsrc.p, S.pval.p, S.rval.p);
  hipLaunchKernelGGL(k_sagg_sum_products, dim3(grid_cap(S.tnnz, VB, 1 << 16)), dim3(VB), 0, s, S.tnnz, S.tseg.p, S.tsrc.p, f->vals.p,
                     S.pval.p, S.tval.p);
  hipLaunchKernelGGL(k_sagg_sum_products, dim3(grid_cap(S.cnnz, VB, 1 << 16)), dim3(VB), 0, s, S.cnnz, S.cseg.p, S.csrc.p, S.tval.p,
                     S.pval.p, c->vals.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

// the values of P, R, T and of A_c (into c->vals) from f's matrix values on the kept term lists
static int sagg_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, double omega, zzz_ctx* c)
{
  hipStream_t s = ctx->stream;
  const int gp = grid_cap(S.pnnz, VB, 1 << 16);
  const int32_t* agg = agg_map(S.agg);
  sagg_diagonal(ctx, f, S);
  if (S.bs == 3)
    hipLaunchKernelGGL(k_sagg_p_values<3>, dim3(gp), dim3(VB), 0, s, S.pnnz, S.pseg.p, S.psrc.p, f->vals.p, S.pfrow.p, S.pcol.p, agg,
                       S.diag.p, omega, S.pval.p);
  else
    hipLaunchKernelGGL(k_sagg_p_values<1>, dim3(gp), dim3(VB), 0, s, S.pnnz, S.pseg.p, S.psrc.p, f->vals.p, S.pfrow.p, S.pcol.p, agg,
                       S.diag.p, omega, S.pval.p);
  return sagg_product_values(ctx, f, S, c);
}

int sagg_galerkin(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c, int level)
{
  int max_row = 0;
  if (ctx->mg_products == ZZZ_MG_PRODUCTS_ROWS)
  {
    S->bs = f->bs;
    S->nf = f->n_owned * f->bs;
    S->nc = agg_count(S->agg) * f->bs;
    if (int rc = sagg_rows_build(ctx, f, *S, SaggPt::UNIT, omega, c, level, &max_row))
      return rc;
  }
  else
  {
    if (int rc = f->bs == 3 ? sagg_structure_bs<3>(ctx, f, *S, c, level, &max_row) : sagg_structure_bs<1>(ctx, f, *S, c, level, &max_row))
      return rc;
    if (int rc = sagg_values(ctx, f, *S, omega, c))
      return rc;
  }
  if (int rc = ctx_adopt_csr(c, S->bs, S->nc / S->bs, S->cnnz, max_row))
    return fail(ctx, rc, "-pc_type sagg: the coarse level of %lld dofs: %s", (long long)S->nc, c->err.c_str());
  return ZZZ_OK;
}

int sagg_refresh(zzz_ctx* ctx, zzz_ctx* f, SaggLevel* S, double omega, zzz_ctx* c)
{
  if (int rc = S->rows ? sagg_rows_values(ctx, f, *S, SaggPt::UNIT, omega, c) : sagg_values(ctx, f, *S, omega, c))
    return rc;
  return ctx_adopt_values(c);
}

template <typename T>
static int64_t sagg_bytes(const DevBuf<T>& b) { return b.p ? (int64_t)(b.cap * sizeof(T)) : 0; }
void sagg_products_info(const SaggLevel* S, int64_t out[8])
{
  for (int i = 0; i < 8; ++i)
    out[i] = 0;
  out[0] = S->rows ? 1 : 0;
  out[1] = sagg_bytes(S->prow) + sagg_bytes(S->pcol) + sagg_bytes(S->pfrow) + sagg_bytes(S->pseg) + sagg_bytes(S->psrc) + sagg_bytes(S->pval)
           + sagg_bytes(S->diag) + sagg_bytes(S->rrow) + sagg_bytes(S->rfine) + sagg_bytes(S->rsrc) + sagg_bytes(S->rval)
           + sagg_bytes(S->tseg) + sagg_bytes(S->cseg) + sagg_bytes(S->tsrc) + sagg_bytes(S->csrc) + sagg_bytes(S->tval)
           + sagg_bytes(S->trow) + sagg_bytes(S->tcol) + sagg_bytes(S->ord);
  out[2] = S->ri.chunks;
  out[3] = S->ri.max_cand;
  out[4] = S->ri.budget;
  out[5] = S->ri.lone;
  out[6] = S->ri.peak;
}

int sagg_restrict(zzz_ctx* ctx, const int* stop, const SaggLevel* S, const double* rf, const double* sub, double* rc)
{
  hipLaunchKernelGGL(k_sagg_restrict, dim3(grid_cap(S->nc, VB / 64, 1 << 20)), dim3(VB), 0, ctx->stream, stop, S->nc, S->rrow.p, S->rfine.p,
                     S->rval.p, rf, sub, rc);
  return ZZZ_OK;
}

int sagg_prolong(zzz_ctx* ctx, const int* stop, const SaggLevel* S, const double* ec, double* xf, int accumulate)
{
  hipLaunchKernelGGL(k_sagg_prolong, dim3(grid_cap(S->nf, VB, 1 << 16)), dim3(VB), 0, ctx->stream, stop, S->nf, S->prow.p, S->pcol.p,
                     S->pval.p, ec, xf, accumulate);
  return ZZZ_OK;
}

// P to the host, the rows of a level in an internal order (level 0 alone) put into the caller's
int sagg_download_p(zzz_ctx* ctx, zzz_ctx* f, const SaggLevel* S, int64_t* rowptr, int32_t* cols, double* vals)
{
  const size_t nf = (size_t)S->nf, nnz = (size_t)S->pnnz;
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!f->dofmap.renumbered)
  {
    if (rowptr)
      ZZZ_HIP(ctx, hipMemcpy(rowptr, S->prow.p, (nf + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (cols)
      ZZZ_HIP(ctx, hipMemcpy(cols, S->pcol.p, nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vals)
      ZZZ_HIP(ctx, hipMemcpy(vals, S->pval.p, nnz * sizeof(double), hipMemcpyDeviceToHost));
    return ZZZ_OK;
  }
  std::vector<rp_t> rp(nf + 1), rpc(nf + 1, 0);
  std::vector<int32_t> cl(nnz);
  std::vector<double> vl(nnz);
  ZZZ_HIP(ctx, hipMemcpy(rp.data(), S->prow.p, (nf + 1) * sizeof(rp_t), hipMemcpyDeviceToHost));
  ZZZ_HIP(ctx, hipMemcpy(cl.data(), S->pcol.p, nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
  ZZZ_HIP(ctx, hipMemcpy(vl.data(), S->pval.p, nnz * sizeof(double), hipMemcpyDeviceToHost));
  const int bs = S->bs;
  auto caller = [&](size_t i) { return (size_t)f->h_perm[i / (size_t)bs] * (size_t)bs + i % (size_t)bs; };
  for (size_t i = 0; i < nf; ++i)
    rpc[caller(i) + 1] = rp[i + 1] - rp[i];
  for (size_t i = 0; i < nf; ++i)
    rpc[i + 1] += rpc[i];
  for (size_t i = 0; i < nf; ++i)
  {
    const size_t o = (size_t)rpc[caller(i)];
    for (rp_t q = rp[i]; q < rp[i + 1]; ++q)
    {
      if (cols)
        cols[o + (size_t)(q - rp[i])] = cl[(size_t)q];
      if (vals)
        vals[o + (size_t)(q - rp[i])] = vl[(size_t)q];
    }
  }
  if (rowptr)
    for (size_t i = 0; i <= nf; ++i)
      rowptr[i] = rpc[i];
  return ZZZ_OK;
}
ZZZ_PRELOAD_TU(sagg)
} // namespace zzz
