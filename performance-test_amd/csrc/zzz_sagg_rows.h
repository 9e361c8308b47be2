// The row-by-row products of ZZZ_MG_PRODUCTS_ROWS (zzz_sagg_rows.hip): what its kernels, its host code and a stand-alone host
// program (tools/sagg_rows_host.cpp, under the sanitizers) share.  Host-compilable, as zzz_mf_elem.h is.
//   * the chunk partition of the symbolic pass: rows are taken in chunks whose candidate count stays within a budget.  The
//     counts are 64-bit prefix sums (a 10 M-dof level has several 10^8 candidates per product); a chunk ends on a row boundary
//     and holds at least one row, so a row that exceeds the budget alone is a chunk of its own;
//   * the search of a column in the sorted columns of an output row, which gives a term its accumulator;
//   * one step of the rule's sum: a plain double addition of an individually rounded product, never fused.
#pragma once
#include <cstdint>

#if !defined(ZZZ_HD)
#if defined(__HIPCC__)
#define ZZZ_HD __host__ __device__
#else
#define ZZZ_HD
#endif
#endif

namespace zzz
{
// the first i in [lo, hi) with a[i] > v, hi when there is none (a ascending)
template <typename T>
ZZZ_HD inline int64_t srow_upper_bound(const T* a, int64_t lo, int64_t hi, T v)
{
  while (lo < hi)
  {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a[mid] > v)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The end r1 of the chunk that starts at row r0 < nrows: the most rows [r0, r1) whose candidates cum[r1] - cum[r0] stay within
// budget >= 1, and r0 + 1 when row r0 alone exceeds it.  cum[0 .. nrows]: the exclusive prefix sums of the rows' candidate
// counts (ascending, not strictly: empty rows).
ZZZ_HD inline int64_t srow_chunk_end(const int64_t* cum, int64_t nrows, int64_t r0, int64_t budget)
{
  const int64_t r1 = srow_upper_bound<int64_t>(cum, r0 + 1, nrows + 1, cum[r0] + budget) - 1;
  return r1 > r0 ? r1 : r0 + 1;
}

// the position of column c among the n ascending, distinct columns of a row; -1 when it is not there
ZZZ_HD inline int32_t srow_find(const int32_t* cols, int32_t n, int32_t c)
{
  int32_t lo = 0, hi = n;
  while (lo < hi)
  {
    const int32_t mid = lo + (hi - lo) / 2;
    if (cols[mid] < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && cols[lo] == c ? lo : -1;
}

// acc + a b in two roundings
ZZZ_HD inline double srow_add(double acc, double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double p = a * b;
  return acc + p;
}
} // namespace zzz
