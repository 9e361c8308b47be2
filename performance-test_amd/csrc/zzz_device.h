// Device helpers shared by the kernel files.
#pragma once
#include <climits>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "zzz_internal.h"

namespace zzz
{
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef int int2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

// Non-temporal access for data touched once per iteration pays only when the working set of the loop exceeds the
// 256 MiB Infinity Cache; a loop that fits (the 8-GPU per-rank size: ~100 MB of operator stream + 60 MB of vectors)
// keeps everything on-die with plain accesses.
template <bool NT, typename T>
__device__ inline T vload(const T* p)
{
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT, typename T>
__device__ inline void vstore(T v, T* p)
{
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// Sum over the workgroup; the result is valid in thread 0.  Fixed tree => reproducible.
__device__ inline double block_reduce_sum(double v, double* sh /* >= blockDim.x/64 doubles of LDS */)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0)
    sh[wv] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i)
      s += sh[i];
  return s;
}

// wave-wide minimum in every lane's hands (a scalar): an inclusive min-scan inside the rows of 16 lanes with DPP
// row shifts, two row broadcasts, then lane 63 read out -- thirteen vector instructions, no LDS crossbar
__device__ inline int wave_min_i(int v)
{
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x111, 0xf, 0xf, false)); // row_shr:1
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x112, 0xf, 0xf, false)); // row_shr:2
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x114, 0xf, 0xf, false)); // row_shr:4
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x118, 0xf, 0xf, false)); // row_shr:8
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x142, 0xa, 0xf, false)); // row_bcast:15 into rows 1, 3
  v = min(v, __builtin_amdgcn_update_dpp(INT_MAX, v, 0x143, 0xc, 0xf, false)); // row_bcast:31 into rows 2, 3
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ inline int wave_max_i(int v) { return -wave_min_i(-v); } // |v| < 2^31 - 1 here

// XCD-aware work mapping for one-shot grids: workgroups are dealt round-robin over the 8 XCDs
// (blockIdx % 8 shares an XCD, MI355X_MICROARCH.md "Workgroup dispatch"), so give XCD x the x-th
// contiguous eighth of the `n` work items: neighbouring items then share that XCD's L2.  Launch
// with xcd_grid(n) workgroups; returns -1 for the few surplus ones.  Placement only changes speed.
__host__ __device__ inline int64_t xcd_grid(int64_t n) { return (n + 7) / 8 * 8; }
__device__ inline int64_t xcd_item(int64_t n)
{
  const int xcd = blockIdx.x & 7;
  const int64_t lo = n * xcd / 8, hi = n * (xcd + 1) / 8;
  const int64_t t = lo + (blockIdx.x >> 3);
  return t < hi ? t : -1;
}
// The same for persistent (grid-stride) kernels: item of step i for this workgroup, -1 when its XCD's eighth is
// exhausted.  Launch with a multiple of 8 workgroups.
__device__ inline int64_t xcd_stride_item(int64_t n, int i)
{
  const int b = blockIdx.x, nb = gridDim.x;
  const int xcd = b & 7;
  const int64_t lo = n * xcd / 8, hi = n * (xcd + 1) / 8;
  const int wg_in_xcd = b >> 3, n_in_xcd = (nb + 7 - xcd) >> 3;
  const int64_t t = lo + wg_in_xcd + (int64_t)i * n_in_xcd;
  return t < hi ? t : -1;
}

// ---- what follows a row's sum in the product kernels (zzz_spmv.hip, zzz_sellp*.hip) ------------------------------------------
// The sums a product leaves beside y, one set per thread: <x, A x>, and for single-reduction CG (x = z) also <r, x> and the
// test norm (<r, r> when nn_is_rr, else <x, x>).  The last term of a Chebyshev product leaves <r, z> and the norm in the same
// two places and no `dot`.
struct RowSums
{
  double dot = 0.0, dot_rx = 0.0, dot_nn = 0.0;
};

// <r, x> and the test norm of a row; nn_is_rr is read here and nowhere else
__device__ __forceinline__ void norm_sums(RowSums& S, const int& nn_is_rr, double xr, double rr)
{
  S.dot_rx += rr * xr;
  S.dot_nn += nn_is_rr ? rr * rr : xr * xr;
}

// A row's terms: its sum (A x)_r, x_r, and r_r where sr.  sr is a template flag of the caller's or a run-time value (the
// tile and generic kernels' rvec != nullptr): inlined, a constant folds and no branch is left.  rr is r_r itself, or
// something to call for it: the two kernels with the run-time flag load r_r only where there is a residual vector.
// The CALLER keeps a lane without a row out (r >= 0 and the like): such a lane may hold 0 * inf.
template <typename RR>
__device__ __forceinline__ void row_sums(RowSums& S, bool sr, const int& nn_is_rr, double sum, double xr, RR rr)
{
  S.dot += sum * xr;
  if (sr)
  {
    if constexpr (std::is_invocable_v<RR>)
      norm_sums(S, nn_is_rr, xr, rr());
    else
      norm_sums(S, nn_is_rr, xr, rr);
  }
}

// One term of the Chebyshev-Jacobi polynomial, w = (A d)_i given: g_i - D^-1_ii w_i and the next d_i.  The only copy of this
// arithmetic: the products' epilogues (cheb_row) and k_cheb_step (zzz_cg.hip: the preconditioner's terms and the multigrid
// smoother's) call it, so the fused and unfused forms of a solver round alike, and like the oracle.
__device__ __forceinline__ void cheb_term(double dinv, double w, double g, double d, double c1, double c2, double& gi, double& dn)
{
  gi = -1.0 * (dinv * w) + g;
  dn = c1 * d + c2 * gi; // (built with -ffp-contract=off: rounded as written, here and in the oracle)
}

// The term as the epilogue of the product of d (ChebEpi, zzz_internal.h): row r's sum is w, xr = d_r, y takes the next d;
// z_r += d'_r.  DOT marks the last term: g and d are left alone, <r, z> and the norm are summed, nothing stored but z.
template <bool DOT>
__device__ __forceinline__ void cheb_row(RowSums& S, const ChebEpi& epi, const int& nn_is_rr, int r, double sum, double xr,
                                         double* __restrict__ y)
{
  double gi, dn;
  cheb_term(epi.dinv[r], sum, epi.g[r], xr, epi.c1, epi.c2, gi, dn);
  const double zi = epi.z[r] + dn;
  epi.z[r] = zi;
  if (DOT)
    norm_sums(S, nn_is_rr, zi, epi.r[r]);
  else
  {
    epi.g[r] = gi;
    y[r] = dn;
  }
}

// The workgroup's partial sums, reduced in the order dot, dot_rx, dot_nn (every thread of the workgroup calls this): dot at
// partials[b] unless the product is a Chebyshev term, the other two at strides 1 and 2 where sr or cheb.
__device__ __forceinline__ void row_sums_store(const RowSums& S, bool sr, bool cheb, double* __restrict__ partials,
                                               const int& pstride, double* red /* as block_reduce_sum's */)
{
  const double sres = cheb ? 0.0 : block_reduce_sum(S.dot, red);
  double s1 = 0.0, s2 = 0.0;
  if (sr || cheb)
  {
    s1 = block_reduce_sum(S.dot_rx, red);
    s2 = block_reduce_sum(S.dot_nn, red);
  }
  if (threadIdx.x == 0)
  {
    if (!cheb)
      partials[blockIdx.x] = sres;
    if (sr || cheb)
    {
      partials[pstride + blockIdx.x] = s1;
      partials[2 * pstride + blockIdx.x] = s2;
    }
  }
}
} // namespace zzz
