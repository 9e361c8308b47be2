// ZZZ_MG_PRODUCTS_ROWS: the products of ZZZ_PC_SAGG and ZZZ_PC_SAGG_RBM -- P = (I - omega D^-1 A) P_t, T = A P, A_c = P^T T -- formed
// row by row.  The lists mode (zzz_sagg.hip) writes every term out with a 64-bit key and a 64-bit value, sorts the lot and keeps
// the sorted lists for the refresh: one to two orders of magnitude more than the entries they produce.  Here nothing of a term
// is kept.  The sums are the same sums (include/zzz_abi.h under ZZZ_PC_SAGG / ZZZ_PC_SAGG_RBM stays the rule): from +0.0, plain
// double additions of individually rounded products, the summation index ascending -- the caller's numbering on level 0, the
// level's own below -- so both modes give the same P, R, T, A_c bit for bit.
//
// One engine, C = L B, used three times per level:
//   P    L = A (rows of constrained dofs skipped), B = P_t.  P_t is never stored: a source (SrowUnitPt: one entry 1 per
//        unconstrained dof of an aggregate; SrowRbmPt: the kept columns of Q) gives its rows to the symbolic pass, and P's
//        value kernels read the aggregate map (and qt) directly.
//   T    L = A, B = P.
//   A_c  L = R = P^T with ascending fine index (so the summation index is the fine row), B = T; the unit diagonal of a dropped
//        coarse dof of ZZZ_PC_SAGG_RBM is one more candidate (d, d) and one term 1.0 x 1.0 of its row.
// On level 0 of a context with an internal dof order L = A is walked through `ord`: the entries of every stored row in
// ascending caller column (one 32-bit permutation, kept).
//
// Symbolic pass (the pattern of C): the candidate count of a row is the sum over its entries of L of the length of B's row;
// the counts' 64-bit prefix sums go to the host, which cuts the rows into chunks within a budget (srow_chunk_end,
// zzz_sagg_rows.h; ZZZ_SAGG_ROWS_BUDGET lowers it).  Per chunk: a wavefront per row writes the candidates as keys
// row << cb | column (cb: the bits of a column), a keys-only radix sort over the bits in use brings them in order, heads + scan
// count the unique ones.  The chunks are walked twice: the first pass only counts, so that the columns get one array of their
// exact size; the second forms every chunk again, compacts its unique keys and writes its row pointers and columns in place
// (a product of one chunk is not formed twice: it still stands in the work buffers).  Nothing of a chunk survives it, and no
// pass allocates inside its loop: the work buffers are sized once, by the largest chunk -- at most 40 B per candidate (two
// keys, head, position, sort scratch), 2 GiB at the default budget whatever the level's size, more only for a row that
// exceeds the budget alone.  The price is every sort run twice where there are several chunks.
//
// Numeric pass (also the whole refresh): a wavefront per output row, one accumulator per output entry -- in LDS where the row
// fits (SROW_LDS_ROW doubles per wavefront, 32 KiB per workgroup of four: five workgroups per CU), in the output array itself
// where it does not.  The row's entries of L are walked in order, one at a time: within one k the entries of B's row k have
// distinct columns, so the lanes take them side by side, each finds its accumulator by binary search in the sorted output
// row (srow_find) and adds its product.  Lanes of ONE wavefront alone ever touch an accumulator, an entry of L after the
// other: no atomics, one fixed order.  A refresh runs no sort and allocates nothing.
#include "zzz_sagg.h"
#include "zzz_sagg_rows.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace zzz
{
constexpr int SROW_LDS_ROW = 1024;                                 // accumulators a wavefront holds in LDS
constexpr int64_t SROW_CAND_BYTES = 40;                            // transient bytes per candidate of a chunk
constexpr int64_t SROW_BUDGET = (2ll << 30) / SROW_CAND_BYTES;     // candidates per chunk: 2 GiB of transient buffers
constexpr int64_t SROW_MAX_CHUNK = (int64_t)INT32_MAX - 16;        // 32-bit positions inside one chunk
constexpr int64_t SROW_MAX_ENTRIES = (int64_t)INT32_MAX;           // entries of A, P, T, A_c: below 2^31

// ---- the rows of B as the symbolic pass reads them -------------------------------------------------------------------
struct SrowCsr
{
  const rp_t* row;
  const int32_t* col;
  __device__ int len(int32_t k) const { return (int)(row[k + 1] - row[k]); }
  __device__ int32_t col_at(int32_t k, int j) const { return col[row[k] + j]; }
};
// ZZZ_PC_SAGG's P_t: 1 from each unconstrained scalar dof (i, c) of an aggregate to (aggregate(i), c)
struct SrowUnitPt
{
  const int32_t* agg;
  const uint8_t* bc;
  int bs;
  __device__ int len(int32_t k) const { return agg[k / bs] >= 0 && bc[k] == 0 ? 1 : 0; }
  __device__ int32_t col_at(int32_t k, int) const { return agg[k / bs] * bs + k % bs; }
};
// ZZZ_PC_SAGG_RBM's P_t: the kept columns q of the aggregate of the dof's node, ascending
struct SrowRbmPt
{
  const int32_t* agg;
  const uint8_t* bc;
  const int32_t* drop;
  int ns;
  __device__ int len(int32_t k) const
  {
    const int32_t J = agg[k / ns];
    if (J < 0 || bc[k] != 0)
      return 0;
    int n = 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
      n += drop[(int64_t)J * RBM_NCOL + q] ? 0 : 1;
    return n;
  }
  __device__ int32_t col_at(int32_t k, int j) const
  {
    const int32_t J = agg[k / ns];
    int32_t col = 0;
    int n = 0;
#pragma unroll
    for (int q = 0; q < RBM_NCOL; ++q)
    {
      const bool kept = !drop[(int64_t)J * RBM_NCOL + q];
      col = kept && n == j ? J * RBM_NCOL + q : col;
      n += kept ? 1 : 0;
    }
    return col;
  }
};

// what one wavefront's lanes have written is read by its other lanes in the next step (LDS or memory)
__device__ inline void srow_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// level 0 in an internal order: entry k of stored row r under (r, column in the caller's numbering)
__global__ __launch_bounds__(VB) void k_srow_ord_keys(int64_t nrows, int bs, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                      const int32_t* __restrict__ perm, u64* __restrict__ key, int32_t* __restrict__ val)
{
  SAGG_FOR(r, nrows)
    for (rp_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
    {
      const int32_t c = cols[k];
      key[k] = ((u64)r << 32) | ((u64)perm[c / bs] * (u64)bs + (u64)(c % bs));
      val[k] = (int32_t)k;
    }
}

// cand[r] = the candidates of row r: the lengths of B's rows over its entries of L (+ 1: a unit diagonal); cand[nrows] = 0
template <typename Src>
__global__ __launch_bounds__(VB) void k_srow_count(int64_t nrows, const rp_t* __restrict__ lrow, const int32_t* __restrict__ lidx,
                                                   const uint8_t* __restrict__ skip, const int32_t* __restrict__ unit, Src src,
                                                   int64_t* __restrict__ cand)
{
  SAGG_FOR(r, nrows + 1)
  {
    int64_t n = 0;
    if (r < nrows && !(skip && skip[r] != 0))
    {
      for (rp_t t = lrow[r]; t < lrow[r + 1]; ++t)
        n += src.len(lidx[t]);
      n += unit && unit[r] ? 1 : 0;
    }
    cand[r] = n;
  }
}

// ... written out for the rows [r0, r1) of a chunk, a wavefront per row: key[cum[r] - cum[r0] ..] = r << cb | column
template <typename Src>
__global__ __launch_bounds__(VB) void k_srow_candidates(int64_t r0, int64_t r1, const rp_t* __restrict__ lrow, const int32_t* __restrict__ lidx,
                                                        const uint8_t* __restrict__ skip, const int32_t* __restrict__ unit, Src src,
                                                        const int64_t* __restrict__ cum, int cb, u64* __restrict__ key)
{
  const int lane = threadIdx.x & 63;
  const int64_t base = cum[r0];
  for (int64_t r = r0 + blockIdx.x * (int64_t)(VB / 64) + (threadIdx.x >> 6); r < r1; r += (int64_t)gridDim.x * (VB / 64))
  {
    if (skip && skip[r] != 0)
      continue;
    int64_t o = cum[r] - base;
    const int64_t end = cum[r + 1] - base;
    const u64 R = (u64)r << cb;
    for (rp_t t = lrow[r]; t < lrow[r + 1]; ++t)
    {
      const int32_t k = lidx[t];
      const int n = src.len(k);
      for (int j = lane; j < n; j += 64)
        if (o + j < end)
          key[o + j] = R | (u64)(unsigned)src.col_at(k, j);
      o += n;
    }
    if (unit && unit[r] && lane == 0 && o < end)
      key[o] = R | (u64)r;
  }
}

// head[t] = sorted key t opens a run of equal keys; head[n] = 0
__global__ __launch_bounds__(VB) void k_srow_heads(int64_t n, const u64* __restrict__ key, int32_t* __restrict__ head)
{
  SAGG_FOR(t, n + 1)
    head[t] = t < n && (t == 0 || key[t - 1] != key[t]) ? 1 : 0;
}

// the unique keys, in order: ukey[pos[t]] = key[t] of every head
__global__ __launch_bounds__(VB) void k_srow_compact(int64_t n, const u64* __restrict__ key, const int32_t* __restrict__ head,
                                                     const int32_t* __restrict__ pos, u64* __restrict__ ukey)
{
  SAGG_FOR(t, n)
    if (head[t])
      ukey[pos[t]] = key[t];
}

// the chunk's part of the CSR from its nu unique keys: col[t] of every key, and crow[s] = base + (keys of rows before s) for
// the rows s = r0 .. r1 (nu = 0: every one is base)
__global__ __launch_bounds__(VB) void k_srow_rows(int64_t nu, const u64* __restrict__ ukey, int cb, int64_t r0, int64_t r1, int64_t base,
                                                  rp_t* __restrict__ crow, int32_t* __restrict__ col)
{
  SAGG_FOR(t, nu + 1)
  {
    int64_t a = t == 0 ? r0 - 1 : (int64_t)(ukey[t - 1] >> cb);
    int64_t b = t == nu ? r1 : (int64_t)(ukey[t] >> cb);
    a = a < r0 - 1 ? r0 - 1 : a;
    b = b > r1 ? r1 : b;
    for (int64_t s = a + 1; s <= b; ++s)
      crow[s] = (rp_t)(base + t);
    if (t < nu)
      col[t] = (int32_t)(ukey[t] & ((1ull << cb) - 1ull));
  }
}

// ZZZ_PC_SAGG:  P(i, J) = delta - (omega s) / a_ii, s the a_ik of the unconstrained k that P_t maps to J, added in ascending k
// (a_ik x 1 is a_ik).  A wavefront per row of P, a lane per entry; every lane walks the row of A.
__global__ __launch_bounds__(VB) void k_srow_p_values_unit(int64_t nf, int bs, const rp_t* __restrict__ arow, const int32_t* __restrict__ acol,
                                                           const double* __restrict__ aval, const int32_t* __restrict__ ord,
                                                           const uint8_t* __restrict__ bc, const int32_t* __restrict__ agg,
                                                           const rp_t* __restrict__ prow, const int32_t* __restrict__ pcol,
                                                           const double* __restrict__ diag, double omega, double* __restrict__ pval)
{
  const int lane = threadIdx.x & 63;
  for (int64_t i = blockIdx.x * (int64_t)(VB / 64) + (threadIdx.x >> 6); i < nf; i += (int64_t)gridDim.x * (VB / 64))
  {
    const rp_t p0 = prow[i], p1 = prow[i + 1];
    if (p0 == p1)
      continue;
    const rp_t a0 = arow[i], a1 = arow[i + 1];
    const int32_t own = agg[i / bs] * bs + (int32_t)(i % bs);
    const double d = diag[i];
    for (rp_t e = p0 + lane; e < p1; e += 64)
    {
      const int32_t col = pcol[e];
      double s = 0.0;
      for (rp_t t = a0; t < a1; ++t)
      {
        const rp_t k = ord ? (rp_t)ord[t] : t;
        const int32_t c = acol[k];
        const double a = aval[k];
        const int32_t J = agg[c / bs];
        const bool hit = J >= 0 && bc[c] == 0 && J * bs + c % bs == col;
        s = hit ? s + a : s;
      }
      const double delta = col == own ? 1.0 : 0.0;
      pval[e] = delta - (omega * s) / d;
    }
  }
}

// ZZZ_PC_SAGG_RBM:  P(i, (J, q)) = P_t(i, (J, q)) - (omega s) / a_ii, s = sum_k a_ik P_t(k, (J, q)) over the unconstrained k of
// aggregate J in ascending k; P_t(k, (J, q)) is qt[q][member row of k]
__global__ __launch_bounds__(VB) void k_srow_p_values_rbm(int64_t nf, int ns, const rp_t* __restrict__ arow, const int32_t* __restrict__ acol,
                                                          const double* __restrict__ aval, const int32_t* __restrict__ ord,
                                                          const uint8_t* __restrict__ bc, const int32_t* __restrict__ agg,
                                                          const int32_t* __restrict__ pos, const double* __restrict__ qt,
                                                          const rp_t* __restrict__ prow, const int32_t* __restrict__ pcol,
                                                          const double* __restrict__ diag, double omega, double* __restrict__ pval)
{
  const int lane = threadIdx.x & 63;
  for (int64_t i = blockIdx.x * (int64_t)(VB / 64) + (threadIdx.x >> 6); i < nf; i += (int64_t)gridDim.x * (VB / 64))
  {
    const rp_t p0 = prow[i], p1 = prow[i + 1];
    if (p0 == p1)
      continue;
    const rp_t a0 = arow[i], a1 = arow[i + 1];
    const int32_t inode = (int32_t)(i / ns);
    const int32_t iagg = agg[inode];
    const int64_t irow = (int64_t)pos[inode] * ns + (i - (int64_t)inode * ns);
    const double d = diag[i];
    for (rp_t e = p0 + lane; e < p1; e += 64)
    {
      const int32_t col = pcol[e];
      const int32_t J = col / RBM_NCOL, q = col - J * RBM_NCOL;
      const double* __restrict__ qq = qt + (int64_t)q * nf;
      double s = 0.0;
      for (rp_t t = a0; t < a1; ++t)
      {
        const rp_t k = ord ? (rp_t)ord[t] : t;
        const int32_t c = acol[k];
        const int32_t node = c / ns;
        if (agg[node] == J && bc[c] == 0)
          s = srow_add(s, aval[k], qq[(int64_t)pos[node] * ns + (c - node * ns)]);
      }
      double pt = 0.0;
      if (iagg == J) // (then node i is a member and irow its place in qt)
        pt = qq[irow];
      pval[e] = pt - (omega * s) / d;
    }
  }
}

// the accumulators of one output row: the entries of L in order, the entries of B's row side by side
__device__ inline void srow_accumulate(double* acc, const int32_t* __restrict__ cc, int32_t n, int lane, rp_t l0, rp_t l1,
                                       const int32_t* __restrict__ lidx, const double* __restrict__ lval, const int32_t* __restrict__ lord,
                                       const rp_t* __restrict__ brow, const int32_t* __restrict__ bcol, const double* __restrict__ bval,
                                       int32_t unit_col)
{
  for (int32_t j = lane; j < n; j += 64)
    acc[j] = 0.0;
  srow_wave_sync();
  if (unit_col >= 0 && lane == 0)
  {
    const int32_t p = srow_find(cc, n, unit_col);
    if (p >= 0)
      acc[p] = srow_add(acc[p], 1.0, 1.0);
  }
  srow_wave_sync();
  for (rp_t t = l0; t < l1; ++t)
  {
    const rp_t e = lord ? (rp_t)lord[t] : t;
    const int32_t k = lidx[e];
    const double a = lval[e];
    for (rp_t q = brow[k] + lane; q < brow[k + 1]; q += 64)
    {
      const int32_t p = srow_find(cc, n, bcol[q]);
      if (p >= 0)
        acc[p] = srow_add(acc[p], a, bval[q]);
    }
    srow_wave_sync();
  }
}

// C = L B on C's pattern, a wavefront per row (LDS: VB / 64 x SROW_LDS_ROW doubles = 32 KiB per workgroup).  lds_cap
// (<= SROW_LDS_ROW): rows of more entries accumulate in cval itself.  unit: a row r with unit[r] set gets the term 1.0 x 1.0 at (r, r).
__global__ __launch_bounds__(VB) void k_srow_numeric(int64_t nrows, const rp_t* __restrict__ lrow, const int32_t* __restrict__ lidx,
                                                     const double* __restrict__ lval, const int32_t* __restrict__ lord,
                                                     const uint8_t* __restrict__ skip, const int32_t* __restrict__ unit,
                                                     const rp_t* __restrict__ brow, const int32_t* __restrict__ bcol,
                                                     const double* __restrict__ bval, const rp_t* __restrict__ crow,
                                                     const int32_t* __restrict__ ccol, double* cval, int lds_cap)
{
  __shared__ double lds[VB / 64][SROW_LDS_ROW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t r = blockIdx.x * (int64_t)(VB / 64) + w; r < nrows; r += (int64_t)gridDim.x * (VB / 64))
  {
    const rp_t c0 = crow[r];
    const int32_t n = (int32_t)(crow[r + 1] - c0);
    if (n <= 0 || (skip && skip[r] != 0))
      continue;
    const int32_t unit_col = unit && unit[r] ? (int32_t)r : -1;
    const rp_t l0 = lrow[r], l1 = lrow[r + 1];
    if (n <= lds_cap)
    {
      srow_accumulate(lds[w], ccol + c0, n, lane, l0, l1, lidx, lval, lord, brow, bcol, bval, unit_col);
      for (int32_t j = lane; j < n; j += 64)
        cval[c0 + j] = lds[w][j];
      srow_wave_sync(); // (the next row of this wavefront zeroes them)
    }
    else
      srow_accumulate(cval + c0, ccol + c0, n, lane, l0, l1, lidx, lval, lord, brow, bcol, bval, unit_col);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int64_t srow_env(const char* name, int64_t dflt)
{
  const char* e = getenv(name);
  const long long v = e ? atoll(e) : 0;
  return v >= 1 && v < dflt ? (int64_t)v : dflt;
}

static int srow_bits(int64_t n) // bits that hold 0 .. n - 1 (at least 1)
{
  int b = 1;
  while (b < 62 && (1ll << b) < n)
    ++b;
  return b;
}

struct SrowWork
{
  DevBuf<int64_t> cand, cum;
  DevBuf<u64> k0, k1;
  DevBuf<int32_t> head, pos;
  DevBuf<unsigned char> tmp;
  int64_t bytes() const
  {
    return (int64_t)((cand.cap + cum.cap) * sizeof(int64_t) + (k0.cap + k1.cap) * sizeof(u64) + (head.cap + pos.cap) * sizeof(int32_t) + tmp.cap);
  }
};

// The pattern of C = L B: crow (nrows + 1) and ccol (*cnnz entries and `pad` zeros behind them).  L's rows: lrow / lidx, rows
// with skip[r] set left out, rows with unit[r] set with one more candidate (r, r); B's rows: src; ncols: C's columns.
template <typename Src>
static int srow_symbolic(zzz_ctx* ctx, SaggLevel& S, int level, const char* what, int64_t nrows, int64_t ncols, const rp_t* lrow,
                         const int32_t* lidx, const uint8_t* skip, const int32_t* unit, Src src, DevBuf<rp_t>& crow, DevBuf<int32_t>& ccol,
                         int64_t pad, int64_t* cnnz)
{
  hipStream_t s = ctx->stream;
  const int64_t budget = S.ri.budget;
  const int cb = srow_bits(ncols), kb = cb + srow_bits(nrows);
  if (kb > 64)
    return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: %lld rows by %lld columns of %s do not fit a 64-bit key", S.tag, level, (long long)nrows,
                (long long)ncols, what);
  SrowWork W;
  ZZZ_HIP(ctx, W.cand.alloc((size_t)nrows + 1));
  ZZZ_HIP(ctx, W.cum.alloc((size_t)nrows + 1));
  ZZZ_HIP(ctx, crow.alloc((size_t)nrows + 1));
  hipLaunchKernelGGL(k_srow_count<Src>, dim3(grid_cap(nrows + 1, VB, 1 << 16)), dim3(VB), 0, s, nrows, lrow, lidx, skip, unit, src, W.cand.p);
  if (int rc = with_scratch(ctx, W.tmp, scan_excl(W.cand.p, W.cum.p, (size_t)nrows + 1, s)))
    return rc;
  std::vector<int64_t> cum((size_t)nrows + 1);
  ZZZ_HIP(ctx, dev_fetch(ctx, W.cum.p, cum.data(), (size_t)nrows + 1));
  // ---- the chunks, from the prefix sums alone; the work buffers are sized once, for the largest ---------------------------
  struct Chunk
  {
    int64_t r0, r1, n, base;
    int32_t nu;
  };
  std::vector<Chunk> chunks;
  int64_t nmax = 0;
  for (int64_t r0 = 0; r0 < nrows;)
  {
    const int64_t r1 = srow_chunk_end(cum.data(), nrows, r0, budget);
    const int64_t n = cum[(size_t)r1] - cum[(size_t)r0];
    if (n > SROW_MAX_CHUNK)
      return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: a row of %s has %lld candidates, 32-bit positions inside a chunk take %lld", S.tag, level,
                  what, (long long)n, (long long)SROW_MAX_CHUNK);
    ++S.ri.chunks;
    if (r1 == r0 + 1 && n > budget)
      ++S.ri.lone;
    for (int64_t r = r0; r < r1; ++r)
      S.ri.max_cand = std::max(S.ri.max_cand, cum[(size_t)r + 1] - cum[(size_t)r]);
    chunks.push_back({r0, r1, n, 0, 0});
    nmax = std::max(nmax, n);
    r0 = r1;
  }
  if (nmax > 0)
  {
    ZZZ_HIP(ctx, W.k0.alloc((size_t)nmax));
    ZZZ_HIP(ctx, W.k1.alloc((size_t)nmax));
    ZZZ_HIP(ctx, W.head.alloc((size_t)nmax + 1));
    ZZZ_HIP(ctx, W.pos.alloc((size_t)nmax + 1));
  }
  // a chunk's candidates sorted into W.k1, the heads of their runs and the heads' positions; ch.nu = the unique ones
  auto unique_chunk = [&](Chunk& ch) -> int {
    ch.nu = 0;
    if (ch.n == 0)
      return ZZZ_OK;
    hipLaunchKernelGGL(k_srow_candidates<Src>, dim3(grid_cap(ch.r1 - ch.r0, VB / 64, 1 << 16)), dim3(VB), 0, s, ch.r0, ch.r1, lrow, lidx, skip,
                       unit, src, W.cum.p, cb, W.k0.p);
    if (int rc = with_scratch(ctx, W.tmp, sort_keys(W.k0.p, W.k1.p, (size_t)ch.n, 0, (unsigned)kb, s)))
      return rc;
    hipLaunchKernelGGL(k_srow_heads, dim3(grid_cap(ch.n + 1, VB, 1 << 16)), dim3(VB), 0, s, ch.n, W.k1.p, W.head.p);
    if (int rc = with_scratch(ctx, W.tmp, scan_excl(W.head.p, W.pos.p, (size_t)ch.n + 1, s)))
      return rc;
    ZZZ_HIP(ctx, dev_fetch(ctx, W.pos.p + ch.n, &ch.nu));
    return ZZZ_OK;
  };
  // ... its unique keys compacted into W.k0, and from them its part of the CSR, in place
  auto write_chunk = [&](const Chunk& ch) -> int {
    if (ch.n > 0)
      hipLaunchKernelGGL(k_srow_compact, dim3(grid_cap(ch.n, VB, 1 << 16)), dim3(VB), 0, s, ch.n, W.k1.p, W.head.p, W.pos.p, W.k0.p);
    hipLaunchKernelGGL(k_srow_rows, dim3(grid_cap((int64_t)ch.nu + 1, VB, 1 << 16)), dim3(VB), 0, s, (int64_t)ch.nu, W.k0.p, cb, ch.r0, ch.r1,
                       ch.base, crow.p, ccol.p + ch.base);
    ZZZ_HIP(ctx, hipGetLastError());
    return ZZZ_OK;
  };
  // ---- first pass: how many entries every chunk has, so that the columns get their array; nothing of a chunk survives it ---
  int64_t total = 0;
  for (Chunk& ch : chunks)
  {
    if (int rc = unique_chunk(ch))
      return rc;
    ch.base = total;
    total += ch.nu;
    if (total >= SROW_MAX_ENTRIES)
      return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: %s has 2^31 entries or more", S.tag, level, what);
  }
  ZZZ_HIP(ctx, ccol.alloc((size_t)(total + pad)));
  // ---- second pass: every chunk again, written in place (one chunk: it still stands in the work buffers) ----------------
  for (Chunk& ch : chunks)
  {
    if (chunks.size() > 1)
      if (int rc = unique_chunk(ch))
        return rc;
    if (int rc = write_chunk(ch))
      return rc;
  }
  if (nrows == 0)
    ZZZ_HIP(ctx, hipMemsetAsync(crow.p, 0, sizeof(rp_t), s));
  if (pad > 0)
    ZZZ_HIP(ctx, hipMemsetAsync(ccol.p + total, 0, (size_t)pad * sizeof(int32_t), s));
  S.ri.peak = std::max(S.ri.peak, W.bytes());
  ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (the work buffers go out of scope)
  *cnnz = total;
  return ZZZ_OK;
}

static void srow_numeric(zzz_ctx* ctx, int64_t nrows, const rp_t* lrow, const int32_t* lidx, const double* lval, const int32_t* lord,
                         const uint8_t* skip, const int32_t* unit, const rp_t* brow, const int32_t* bcol, const double* bval, const rp_t* crow,
                         const int32_t* ccol, double* cval)
{
  // (ZZZ_SAGG_ROWS_LDS lowers the row length that accumulates in LDS: a test reaches the in-memory path on a small mesh)
  const int lds_cap = (int)srow_env("ZZZ_SAGG_ROWS_LDS", SROW_LDS_ROW);
  hipLaunchKernelGGL(k_srow_numeric, dim3(grid_cap(nrows, VB / 64, 1 << 16)), dim3(VB), 0, ctx->stream, nrows, lrow, lidx, lval, lord, skip, unit,
                     brow, bcol, bval, crow, ccol, cval, lds_cap);
}

int sagg_rows_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, SaggPt pt, double omega, zzz_ctx* c)
{
  hipStream_t s = ctx->stream;
  const int32_t* agg = agg_map(S.agg);
  const int32_t* ord = S.ord.p; // (null: the stored order is the caller's)
  const int gw = grid_cap(S.nf, VB / 64, 1 << 16);
  if (int rc = sagg_diagonal(ctx, f, S))
    return rc;
  if (pt == SaggPt::RBM)
    hipLaunchKernelGGL(k_srow_p_values_rbm, dim3(gw), dim3(VB), 0, s, S.nf, S.ns, f->rowptr.p, f->cols.p, f->vals.p, ord, f->bc.p, agg, S.pos.p,
                       S.qt.p, S.prow.p, S.pcol.p, S.diag.p, omega, S.pval.p);
  else
    hipLaunchKernelGGL(k_srow_p_values_unit, dim3(gw), dim3(VB), 0, s, S.nf, S.bs, f->rowptr.p, f->cols.p, f->vals.p, ord, f->bc.p, agg, S.prow.p,
                       S.pcol.p, S.diag.p, omega, S.pval.p);
  sagg_r_values(ctx, S);
  srow_numeric(ctx, S.nf, f->rowptr.p, f->cols.p, f->vals.p, ord, f->bc.p, nullptr, S.prow.p, S.pcol.p, S.pval.p, S.trow.p, S.tcol.p, S.tval.p);
  srow_numeric(ctx, S.nc, S.rrow.p, S.rfine.p, S.rval.p, nullptr, nullptr, S.ndrop > 0 ? S.drop.p : nullptr, S.trow.p, S.tcol.p, S.tval.p,
               c->rowptr.p, c->cols.p, c->vals.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

int sagg_rows_build(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, SaggPt pt, double omega, zzz_ctx* c, int level, int* max_row)
{
  hipStream_t s = ctx->stream;
  const int64_t N = f->nnz, nf = S.nf, nc = S.nc;
  const int32_t* agg = agg_map(S.agg);
  const int32_t* perm = f->dofmap.renumbered ? f->perm.p : nullptr;
  S.rows = true;
  S.ri = SaggLevel::RowsInfo();
  S.ri.budget = srow_env("ZZZ_SAGG_ROWS_BUDGET", SROW_BUDGET);
  if (N >= SROW_MAX_ENTRIES)
    return fail(ctx, ZZZ_ERR_LIMIT, "%s: level %d: A has 2^31 entries or more", S.tag, level);
  // ---- level 0 in an internal order: the entries of every stored row in ascending caller column ---------------------
  S.ord.release();
  if (perm)
  {
    DevBuf<u64> k0, k1;
    DevBuf<int32_t> v0;
    DevBuf<unsigned char> tmp;
    ZZZ_HIP(ctx, k0.alloc((size_t)N));
    ZZZ_HIP(ctx, k1.alloc((size_t)N));
    ZZZ_HIP(ctx, v0.alloc((size_t)N));
    ZZZ_HIP(ctx, S.ord.alloc((size_t)N));
    hipLaunchKernelGGL(k_srow_ord_keys, dim3(grid_cap(nf, VB, 1 << 16)), dim3(VB), 0, s, nf, S.bs, f->rowptr.p, f->cols.p, perm, k0.p, v0.p);
    if (int rc = with_scratch(ctx, tmp, sort_pairs(k0.p, k1.p, v0.p, S.ord.p, (size_t)N, 0, 64, s)))
      return rc;
    ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (the three are locals)
    S.ri.peak = std::max(S.ri.peak, (int64_t)((k0.cap + k1.cap) * sizeof(u64) + v0.cap * sizeof(int32_t) + tmp.cap));
  }
  // ---- P = (I - omega D^-1 A) P_t: the pattern -------------------------------------------------------------------------
  if (int rc = pt == SaggPt::RBM
                   ? srow_symbolic(ctx, S, level, "P", nf, nc, f->rowptr.p, f->cols.p, f->bc.p, nullptr, SrowRbmPt{agg, f->bc.p, S.drop.p, S.ns},
                                   S.prow, S.pcol, 0, &S.pnnz)
                   : srow_symbolic(ctx, S, level, "P", nf, nc, f->rowptr.p, f->cols.p, f->bc.p, nullptr, SrowUnitPt{agg, f->bc.p, S.bs}, S.prow,
                                   S.pcol, 0, &S.pnnz))
    return rc;
  if (S.pnnz <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: the prolongator to %lld coarse dofs is empty", S.tag, level, (long long)nc);
  ZZZ_HIP(ctx, S.pval.alloc((size_t)S.pnnz + 1));
  ZZZ_HIP(ctx, S.diag.alloc((size_t)nf));
  // ---- R = P^T, as the lists mode builds it ----------------------------------------------------------------------------
  {
    SaggWork W;
    DevBuf<int32_t> pfrow;
    ZZZ_HIP(ctx, pfrow.alloc((size_t)S.pnnz));
    sagg_row_index(ctx, nf, S.prow.p, pfrow.p);
    if (int rc = sagg_transpose_p(ctx, S, perm, pfrow.p, W)) // (ends synchronised)
      return rc;
    S.ri.peak = std::max(S.ri.peak, (int64_t)((W.k0.cap + W.k1.cap + W.v0.cap) * sizeof(u64) + W.tmp.cap + pfrow.cap * sizeof(int32_t))
                                        + 12 * S.pnnz);
  }
  // ---- T = A P and A_c = P^T T: the patterns ---------------------------------------------------------------------------
  if (int rc = srow_symbolic(ctx, S, level, "A P", nf, nc, f->rowptr.p, f->cols.p, f->bc.p, nullptr, SrowCsr{S.prow.p, S.pcol.p}, S.trow, S.tcol,
                             0, &S.tnnz))
    return rc;
  ZZZ_HIP(ctx, S.tval.alloc((size_t)S.tnnz + 1));
  if (int rc = srow_symbolic(ctx, S, level, "P^T (A P)", nc, nc, S.rrow.p, S.rfine.p, nullptr, S.ndrop > 0 ? S.drop.p : nullptr,
                             SrowCsr{S.trow.p, S.tcol.p}, c->rowptr, c->cols, 8, &S.cnnz))
    return rc;
  if (S.cnnz <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: the coarse matrix of %lld dofs is empty", S.tag, level, (long long)nc);
  ZZZ_HIP(ctx, c->vals.alloc((size_t)S.cnnz + 8));
  ZZZ_HIP(ctx, hipMemsetAsync(c->vals.p + S.cnnz, 0, 8 * sizeof(double), s));
  DevBuf<int32_t> stats;
  ZZZ_HIP(ctx, stats.alloc(2));
  ZZZ_HIP(ctx, hipMemsetAsync(stats.p, 0, 2 * sizeof(int32_t), s));
  sagg_row_stats(ctx, nc, c->rowptr.p, stats.p);
  int32_t hs[2] = {0, 0};
  ZZZ_HIP(ctx, dev_fetch(ctx, stats.p, hs, 2));
  ZZZ_HIP(ctx, hipGetLastError());
  if (hs[1] > 0)
    return fail(ctx, ZZZ_ERR_ARG, "%s: level %d: %d coarse dofs have no unconstrained member (aggregates of partly "
                                  "constrained block dofs): the coarse matrix would be singular", S.tag, level, hs[1]);
  *max_row = hs[0];
  return sagg_rows_values(ctx, f, S, pt, omega, c);
}
ZZZ_PRELOAD_TU(sagg_rows)
} // namespace zzz
