// Conjugate gradients on the GPU: linalg::cg of src/cg.h:38-86 (variant CGH) and PETSc's KSPCG with
// PCJACOBI / PCNONE as the reference selects it at src/poisson_problem.cpp:168-177 (variant PETSC).
//
// All Krylov scalars live in device memory; the host only enqueues.  One iteration is three kernels:
//   k_update_p : sums the partials of <r,z> and of the test norm left by the previous kernel (every
//                workgroup redundantly, in the same fixed order => identical scalars), does the
//                convergence test (squared_norm + test, src/cg.h:74-79), then
//                x += alpha_{k-1} p  (the previous iteration's axpy, src/cg.h:68, applied here because p
//                is read anyway) and p = z + (beta_k / beta_{k-1}) p    (axpy, src/cg.h:82)
//   [halo]     : ghost values of p from their owners                   (scatter_fwd)
//   spmv       : w = A p, per-workgroup partials of <p, w>             (action, src/cg.h:62)
//   k_update_xr: sums the <p,w> partials -> alpha = beta_k / <p,w>     (inner_product, src/cg.h:65);
//                r -= alpha w; z = D^-1 r; partials of <r,z> and the test norm
//                                                                      (axpy, src/cg.h:71)
// With a communicator attached a one-workgroup reduce + ncclAllReduce sits between producer and
// consumer, and the consumer reads the single all-reduced value instead of the partials.
// Every kernel returns at once when the device-side `converged` flag is set; the host polls that
// flag a few iterations behind the queue, so the returned iteration count is exact.
// Reductions use fixed trees => reproducible runs.
// HBM traffic per iteration beyond the SpMV, in-place loop: 40 B/row (x and p update) + 40 B/row (r, z update); with
// Jacobi's inverse diagonal as codes and z recomputed (DZ) 42 + 26 = 68.  Where the loop runs out of HBM the solution
// update is deferred (ZZZ_CG_XDEFER, k_update_p_light / _flush below): p_k in a ring of K vectors, x read and written
// once per K iterations instead of in every one -- 16 B/row become 8 + 8/K, k_update_p 26 B/row in K - 1 of K launches
// and 34 + 8 K in the K-th: 36 + 26 = 62 B/row on average at the default K = 4.
#include "zzz_device.h"
#include "zzz_internal.h"
#include "zzz_cg.h"

#include <cmath>
#include <cstdlib>

namespace zzz
{
// one workgroup-wide sum of parts[0..np) (fixed order); result in every thread
__device__ inline double reduce_parts_bcast(const double* __restrict__ parts, int np, double* sh)
{
  double s = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x)
    s += parts[i];
  const double t = block_reduce_sum(s, sh);
  __shared__ double bc;
  __syncthreads();
  if (threadIdx.x == 0)
    bc = t;
  __syncthreads();
  return bc;
}

// The scalar logic at the head of iteration `it` (convergence test of the completed iterations and the new
// direction's coefficient), identical in every workgroup; workgroup 0 records it.  pa/pb: partials (or the single
// all-reduced values) of <r,z> and of the test norm.  Returns false when an EARLIER launch has stopped the solve
// (this one must do nothing).  sh: >= blockDim.x/64 doubles of LDS.
struct DirScalars
{
  double rz, bprev;
  int conv;
};
__device__ inline bool cg_direction_scalars(CgState* __restrict__ st, double* __restrict__ beta_hist,
                                            double* __restrict__ dp_hist, int it, const CgParams& P,
                                            const double* __restrict__ pa, const double* __restrict__ pb, int np, double* sh,
                                            DirScalars& S)
{
  // every input of the scalar logic is requested up-front (uniform loads, one round trip): the stop word, the state,
  // last iteration's <r,z>, and -- communicator attached, np == 1 -- the two all-reduced sums themselves
  const int c = __atomic_load_n(&st->conv_it1, __ATOMIC_RELAXED);
  const double dp0_st = st->dp0, ttol_st = st->ttol;
  const double bprev_h = (it == 0) ? 1.0 : beta_hist[it - 1];
  double rz = pa[0], nn = pb[0], unused;
  // stopped by an EARLIER launch (c - 1 < it): that word was written before this launch began, so every wavefront
  // reads the same value and the branch is uniform without a broadcast
  if (c != 0 && c - 1 < it)
    return false;
  if (np != 1)
    reduce_parts3_bcast(pa, pb, nullptr, np, rz, nn, unused);
  // scalar logic, identical in every workgroup; workgroup 0 records it
  double dp, dp0 = dp0_st, ttol = ttol_st;
  int conv = 0;
  if (P.variant == ZZZ_CG_CGH)
  {
    // src/cg.h:53-55,74-79: rnorm = <r,r>; break when rnorm/rnorm0 < rtol^2 (strict), no test at k = 0
    dp = rz;
    if (it == 0)
    {
      dp0 = rz;
      ttol = P.rtol * P.rtol;
    }
    else if (rz / dp0 < P.rtol * P.rtol)
      conv = 1;
  }
  else
  {
    dp = (P.norm == ZZZ_NORM_NATURAL) ? sqrt(fabs(rz)) : sqrt(nn);
    if (it == 0)
    {
      dp0 = dp;
      ttol = fmax(P.rtol * dp, P.atol);
    }
    if (!isfinite(dp))
      conv = 2;
    else if (dp <= ttol) // KSPConvergedDefault
      conv = 1;
    else if (dp >= P.dtol * dp0) // ... KSP_DIVERGED_DTOL
      conv = 3;
  }
  const double bprev = bprev_h;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    beta_hist[it] = rz;
    dp_hist[it] = dp;
    st->dp = dp;
    if (it == 0)
    {
      st->dp0 = dp0;
      st->ttol = ttol;
    }
    if (conv)
    {
      st->iters = it;
      st->converged = conv; // the other workgroups reach the same verdict from the same partials
      __atomic_store_n(&st->conv_it1, it + 1, __ATOMIC_RELAXED);
    }
  }
  S.rz = rz;
  S.bprev = bprev;
  S.conv = conv;
  return true;
}

// Inhomogeneous Dirichlet values with the matrix-free operator (zzz_bc_values_upload): its action zeroes the constrained
// ROWS (src/cgpoisson_problem.cpp:207), so the solve iterates on b with its constrained entries taken as zero -- what
// apply_lifting's scale 0.0 leaves there (:168) -- in a copy: the caller's b keeps b[bc] = g ...
__global__ void k_masked_copy(const double* __restrict__ b, const uint8_t* __restrict__ bc, double* __restrict__ out, int64_t n)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
  {
    const double v = b[r];
    out[r] = bc[r] ? 0.0 : v;
  }
}
// ... and KSPCG, whose iterates keep u[bc] = 0, ends with u[bc] = g (the identity rows of the assembled operator give the same)
__global__ void k_set_bc_values(const uint8_t* __restrict__ bc, const double* __restrict__ g, double* __restrict__ u, int64_t n)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
  {
    const double v = g[r];
    if (bc[r])
      u[r] = v;
  }
}

__global__ void k_invert(double* __restrict__ d, int64_t n)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    d[r] = 1.0 / (d[r] == 0.0 ? 1.0 : d[r]); // PCJACOBI replaces zero diagonal entries by one
}

__global__ void k_extract_dinv(const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                               const double* __restrict__ vals, double* __restrict__ dinv, int64_t n, int jacobi)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
  {
    double d = 1.0;
    if (jacobi)
    {
      // columns are ascending: binary search for the diagonal (MatGetDiagonal)
      int64_t lo = rowptr[r], hi = rowptr[r + 1] - 1;
      d = 0.0;
      while (lo <= hi)
      {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t cm = cols[mid];
        if (cm == (int32_t)r)
        {
          d = vals[mid];
          break;
        }
        if (cm < (int32_t)r)
          lo = mid + 1;
        else
          hi = mid - 1;
      }
      if (d == 0.0)
        d = 1.0; // PCJACOBI replaces zero diagonal entries by one
    }
    dinv[r] = 1.0 / d;
  }
}

// ---- the inverse diagonal as 16-bit codes (DinvCodes below): distinct values of d[0..n) into a set (zzz_valset.h) of
// 16 384 slots for at most DZ_MAX = 2 048 values
constexpr int DD_BITS = decltype(zzz_ctx::dd_set)::bits;
__global__ __launch_bounds__(256) void k_dd_insert(const double* __restrict__ d, int64_t n, unsigned long long* __restrict__ table,
                                                   int* __restrict__ info, int limit)
{
  const int64_t span = (n + 63) & ~(int64_t)63;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < span; i += gridDim.x * 256ll)
  {
    const bool have = i < n;
    const unsigned long long b = have ? (unsigned long long)__double_as_longlong(d[i]) : 0ull;
    if (!valset_insert_wave<DD_BITS>(table, info, limit, b, have))
      return;
  }
}
__global__ __launch_bounds__(256) void k_dd_encode(const double* __restrict__ d, int64_t n, int64_t npad,
                                                   const unsigned long long* __restrict__ table, const int32_t* __restrict__ slot_code,
                                                   uint16_t* __restrict__ codes, const int* __restrict__ info, int allow8)
{
  if (info[1])
    return;
  // one byte per entry when every code fits one (info[2]: the values numbered; dinv_codes_build applies the same rule to
  // the count it reads back)
  const bool b8 = allow8 && info[2] <= DZ8_MAX;
  uint8_t* __restrict__ codes8 = reinterpret_cast<uint8_t*>(codes);
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < npad; i += gridDim.x * 256ll)
  {
    const int c = i < n ? valset_find<DD_BITS>(table, slot_code, (unsigned long long)__double_as_longlong(d[i])) : 0;
    if (b8)
      codes8[i] = (uint8_t)c;
    else
      codes[i] = (uint16_t)c;
  }
}

// r = b - w (w = A x0, or nothing when x0 == 0); z = dinv r; partials: pa = <r,z>, pb = test norm^2
__global__ __launch_bounds__(VB) void k_init_residual(const double* __restrict__ b, const double* __restrict__ w,
                                                      const double* __restrict__ dinv, double* __restrict__ r,
                                                      double* __restrict__ z, int64_t n, int norm,
                                                      double* __restrict__ pa, double* __restrict__ pb)
{
  __shared__ double sh[VB / 64];
  double sa = 0, sb = 0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    const double ri = w ? (-1.0 * w[i] + b[i]) : b[i]; // axpy(r, -1, y, b), src/cg.h:47
    const double zi = dinv[i] * ri;
    r[i] = ri;
    z[i] = zi;
    sa += ri * zi;
    sb += (norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : zi * zi;
  }
  const double ta = block_reduce_sum(sa, sh);
  const double tb = block_reduce_sum(sb, sh);
  if (threadIdx.x == 0)
  {
    pa[blockIdx.x] = ta;
    pb[blockIdx.x] = tb;
  }
}

// `it` = number of completed iterations.  pa/pb: partials of <r,z> and of the test norm (np each).
// The solution update of the PREVIOUS iteration, x += alpha_{it-1} p_{it-1}, is applied here (p is read
// anyway) instead of in k_update_xr: one vector read less per iteration, same operations on the same
// operands, so x is bit-identical.  It must be applied by the launch that detects convergence too; only
// launches enqueued after that one skip it (conv_it1).  update_dir == 0: the final test after max_it.
// DZ (round 4): no z vector.  Jacobi's inverse diagonal holds few distinct values on a regular mesh (a subset of the
// matrix's: section 3 of DESIGN.md); as 16-bit codes into a table in LDS it costs 2 B per row instead of 8, and with it
// z = D^-1 r is cheaper to RECOMPUTE here from r (the same product of the same two doubles: the same bits) than to
// write in k_update_xr and read back: 80 -> 68 B per row and iteration for the two kernels.  dz.codes = nullptr: off.
// With at most 256 distinct values the codes are bytes (DZ = 2 of zzz_cg.h): 1 B per row, 66 B for the two kernels.  The
// table entry a code selects is the same double, so nothing downstream changes.  Each kernel below is one __global__
// template compiled per DZ (0 doubles, 1 16-bit codes, 2 8-bit codes); the drivers pick the instantiation with dz_dispatch.

template <bool NT, int DZ = 0>
__global__ __launch_bounds__(VB) void k_update_p(CgState* __restrict__ st, double* __restrict__ beta_hist,
                                                 double* __restrict__ dp_hist, const double* __restrict__ alpha_hist,
                                                 int it, CgParams P, const double* __restrict__ pa,
                                                 const double* __restrict__ pb, int np, const double* __restrict__ z,
                                                 double* __restrict__ p, double* __restrict__ x, int64_t n,
                                                 int update_dir, DinvCodes dz = DinvCodes())
{
  __shared__ double sh[VB / 64];
  __shared__ double dtab[dz_table(DZ)];
  dz_stage<DZ>(dtab, dz);
  // The first entries of this thread are requested BEFORE the scalar prologue (flag, partial sums, convergence logic: a
  // chain of dependent loads and barriers of 3-5 us that every workgroup walks): at the 8-GPU per-rank size a thread
  // has one or two entries in all, so the kernel was prologue + one memory round trip in sequence (11-12 us for 50 MB
  // that stream in 7).  Clamped index: the loads are unconditional, a thread without entries drops them.
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * VB;
  const int64_t i0 = blockIdx.x * (int64_t)VB + threadIdx.x;
  dbl2* __restrict__ p2 = reinterpret_cast<dbl2*>(p);
  dbl2* __restrict__ x2 = reinterpret_cast<dbl2*>(x);
  const dbl2* __restrict__ z2 = reinterpret_cast<const dbl2*>(DZ ? dz.r : z);
  const int64_t c0 = (i0 < n2) ? i0 : 0;
  dbl2 pi0 = {0, 0}, xi0 = {0, 0}, zi0 = {0, 0};
  uint32_t dc0 = 0;
  if (n2 > 0)
  {
    pi0 = p2[c0];
    xi0 = vload<NT>(x2 + c0);
    zi0 = vload<NT>(z2 + c0); // DZ: r
    if (DZ)
      dc0 = dz_load2<DZ>(dz, c0);
  }
  const double alpha_h = it > 0 ? alpha_hist[it - 1] : 0.0; // requested with the rest of the prologue's inputs
  DirScalars S;
  if (!cg_direction_scalars(st, beta_hist, dp_hist, it, P, pa, pb, np, sh, S))
    return;
  const int conv = S.conv;
  const double rz = S.rz, bprev = S.bprev;
  const bool dir = !conv && update_dir;
  if (it == 0)
  {
    if (dir)
      for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
        p[i] = DZ ? dtab[dz_load1<DZ>(dz, i)] * dz.r[i] : z[i];
    return;
  }
  const double alpha = alpha_h;
  const double bcoef = rz / bprev;
  // two entries per lane and load (16-B accesses); the arithmetic per entry is unchanged
  for (int64_t i = i0; i < n2; i += stride)
  {
    dbl2 pi, xi, zi;
    if (i == i0)
    {
      pi = pi0;
      xi = xi0; // x is touched once per iteration: keep the cache for p, z, w
      zi = zi0; // last use of z
    }
    else
    {
      pi = p2[i];
      xi = vload<NT>(x2 + i);
      zi = vload<NT>(z2 + i);
    }
    if (DZ)
    {
      const uint32_t dc = i == i0 ? dc0 : dz_load2<DZ>(dz, i);
      zi.x = dtab[dz_lo<DZ>(dc)] * zi.x; // z = D^-1 r, as k_update_xr formed it for its sums
      zi.y = dtab[dz_hi<DZ>(dc)] * zi.y;
    }
    xi.x = alpha * pi.x + xi.x; // src/cg.h:68, one kernel late
    xi.y = alpha * pi.y + xi.y;
    vstore<NT>(xi, x2 + i);
    if (dir)
    {
      dbl2 pn;
      pn.x = bcoef * pi.x + zi.x;
      pn.y = bcoef * pi.y + zi.y;
      p2[i] = pn;
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    const int64_t i = n - 1;
    const double pi = p[i];
    x[i] = alpha * pi + x[i];
    if (dir)
      p[i] = bcoef * pi + (DZ ? dtab[dz_load1<DZ>(dz, i)] * dz.r[i] : z[i]);
  }
}

// ---- the solution update deferred (ZZZ_CG_XDEFER): a ring of K direction vectors, x touched once per K iterations ----
// Nothing in the loop reads x, yet k_update_p above reads and writes it in every iteration: 16 of its 42 B per row.
// Here p_k lives in slot k mod K of a ring (slot 0 is ctx->p) and k_update_p comes in two forms:
//   light (k mod K != 0, and k == 0): test and scalars as above, p_k = z_k + beta p_{k-1} from slot (k-1) mod K into
//          slot k mod K.  x is not touched: 26 B per row with DZ.
//   flush (k mod K == 0, k > 0): the same, and per entry the K pending updates x = alpha_j p_j + x, j = k-K .. k-1 in
//          ascending order -- slots 0 .. K-1 in that order, because K divides k.  p_{k-1} is in registers anyway, the
//          older K-1 are read for the last time, and the new p_k overwrites p_{k-K} in slot 0 by the lane that has
//          just read it.  16 + 8 (K-1) B per row more than the light form.
// Every entry of x receives the same multiplies and adds in the same order as in the in-place kernel, only later:
// the same bits.  The launch that detects convergence at iteration c leaves the ring alone like every launch behind
// it (a flush form still applies its updates, as the in-place kernel does), so the flushes that ran are those with
// k mod K == 0 and k <= c, x holds the updates j < K floor(c / K), and slots 0 .. c mod K - 1 hold the directions of
// the rest: k_x_apply_pending, after the loop, reads c on the device and applies them.
constexpr int XD_KMAX = 8;
struct PRing
{
  double* slot[XD_KMAX];
};

template <bool NT, int DZ, int NF> // NF: updates applied by this launch (0: the light form; K: the flush form)
__device__ __forceinline__ void update_p_deferred(CgState* __restrict__ st, double* __restrict__ beta_hist, double* __restrict__ dp_hist,
                                                  const double* __restrict__ alpha_hist, int it, const CgParams& P,
                                                  const double* __restrict__ pa, const double* __restrict__ pb, int np,
                                                  const double* __restrict__ z, const double* pprev, double* pnew, const PRing& ring,
                                                  double* __restrict__ x, int64_t n, int update_dir, const DinvCodes& dz)
{
  __shared__ double sh[VB / 64];
  __shared__ double dtab[dz_table(DZ)];
  dz_stage<DZ>(dtab, dz);
  // first entries requested before the scalar prologue, as in k_update_p (the older directions of a flush are not: they
  // would be K - 1 more 16-B requests per lane for a form that runs once in K iterations)
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * VB;
  const int64_t i0 = blockIdx.x * (int64_t)VB + threadIdx.x;
  const dbl2* pp2 = reinterpret_cast<const dbl2*>(pprev);
  dbl2* pn2 = reinterpret_cast<dbl2*>(pnew);
  dbl2* __restrict__ x2 = reinterpret_cast<dbl2*>(x);
  const dbl2* __restrict__ z2 = reinterpret_cast<const dbl2*>(DZ ? dz.r : z);
  const int64_t c0 = (i0 < n2) ? i0 : 0;
  dbl2 pi0 = {0, 0}, xi0 = {0, 0}, zi0 = {0, 0};
  uint32_t dc0 = 0;
  if (n2 > 0)
  {
    pi0 = pp2[c0];
    if (NF)
      xi0 = vload<NT>(x2 + c0);
    zi0 = vload<NT>(z2 + c0); // DZ: r
    if (DZ)
      dc0 = dz_load2<DZ>(dz, c0);
  }
  double al[NF ? NF : 1]; // alpha_{it-K} .. alpha_{it-1}, requested with the rest of the prologue's inputs
  if (NF)
  {
#pragma unroll
    for (int j = 0; j < NF; ++j)
      al[j] = alpha_hist[it - NF + j];
  }
  DirScalars S;
  if (!cg_direction_scalars(st, beta_hist, dp_hist, it, P, pa, pb, np, sh, S))
    return;
  const bool dir = !S.conv && update_dir;
  if (NF == 0)
  {
    if (!dir)
      return; // nothing but the test: the pending updates are k_x_apply_pending's
    if (it == 0)
    {
      for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
        pnew[i] = DZ ? dtab[dz_load1<DZ>(dz, i)] * dz.r[i] : z[i];
      return;
    }
  }
  const double bcoef = S.rz / S.bprev;
  for (int64_t i = i0; i < n2; i += stride)
  {
    dbl2 pi, xi = {0, 0}, zi;
    if (i == i0)
    {
      pi = pi0;
      xi = xi0;
      zi = zi0;
    }
    else
    {
      pi = pp2[i];
      if (NF)
        xi = vload<NT>(x2 + i);
      zi = vload<NT>(z2 + i);
    }
    if (DZ)
    {
      const uint32_t dc = i == i0 ? dc0 : dz_load2<DZ>(dz, i);
      zi.x = dtab[dz_lo<DZ>(dc)] * zi.x; // z = D^-1 r, as k_update_xr formed it for its sums
      zi.y = dtab[dz_hi<DZ>(dc)] * zi.y;
    }
    if (NF)
    {
#pragma unroll
      for (int j = 0; j < NF - 1; ++j)
      {
        // K = 8: at most four older directions in flight (all seven: 74 registers, six wavefronts per SIMD instead of eight)
        if (j == 4)
          __builtin_amdgcn_sched_barrier(0);
        const dbl2 pj = vload<NT>(reinterpret_cast<const dbl2*>(ring.slot[j]) + i); // last use of p_{it-K+j}
        xi.x = al[j] * pj.x + xi.x; // src/cg.h:68, up to K kernels late
        xi.y = al[j] * pj.y + xi.y;
      }
      xi.x = al[NF - 1] * pi.x + xi.x;
      xi.y = al[NF - 1] * pi.y + xi.y;
      vstore<NT>(xi, x2 + i);
    }
    if (dir)
    {
      dbl2 pn;
      pn.x = bcoef * pi.x + zi.x;
      pn.y = bcoef * pi.y + zi.y;
      pn2[i] = pn;
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    const int64_t i = n - 1;
    const double pi = pprev[i];
    if (NF)
    {
      double xi = x[i];
#pragma unroll
      for (int j = 0; j < NF - 1; ++j)
        xi = al[j] * ring.slot[j][i] + xi;
      x[i] = al[NF - 1] * pi + xi;
    }
    if (dir)
      pnew[i] = bcoef * pi + (DZ ? dtab[dz_load1<DZ>(dz, i)] * dz.r[i] : z[i]);
  }
}

// (two kernels, not one with a flag: a kernel trace tells them apart by name)
template <bool NT, int DZ>
__global__ __launch_bounds__(VB) void k_update_p_light(CgState* __restrict__ st, double* __restrict__ beta_hist, double* __restrict__ dp_hist,
                                                       const double* __restrict__ alpha_hist, int it, CgParams P,
                                                       const double* __restrict__ pa, const double* __restrict__ pb, int np,
                                                       const double* __restrict__ z, const double* pprev, double* pnew, PRing ring,
                                                       double* __restrict__ x, int64_t n, int update_dir, DinvCodes dz)
{
  update_p_deferred<NT, DZ, 0>(st, beta_hist, dp_hist, alpha_hist, it, P, pa, pb, np, z, pprev, pnew, ring, x, n, update_dir, dz);
}
template <bool NT, int DZ, int K>
__global__ __launch_bounds__(VB) void k_update_p_flush(CgState* __restrict__ st, double* __restrict__ beta_hist, double* __restrict__ dp_hist,
                                                       const double* __restrict__ alpha_hist, int it, CgParams P,
                                                       const double* __restrict__ pa, const double* __restrict__ pb, int np,
                                                       const double* __restrict__ z, const double*, double*, PRing ring,
                                                       double* __restrict__ x, int64_t n, int update_dir, DinvCodes dz)
{
  update_p_deferred<NT, DZ, K>(st, beta_hist, dp_hist, alpha_hist, it, P, pa, pb, np, z, ring.slot[K - 1], ring.slot[0], ring, x, n,
                               update_dir, dz);
}

// The updates still pending when the solve has ended: j in [K floor(c / K), c), c = the iteration the solve stopped at
// (st->iters; it_end = max_it when nothing stopped it), p_j in slot j mod K.  The one launch of a solve that runs
// although the stop word is set; the host enqueues it once, without knowing c.
template <int K>
__global__ __launch_bounds__(VB) void k_x_apply_pending(const CgState* __restrict__ st, const double* __restrict__ alpha_hist, int it_end,
                                                        PRing ring, double* __restrict__ x, int64_t n)
{
  const int c = st->converged ? st->iters : it_end;
  const int lo = (c / K) * K, m = c - lo;
  if (m == 0)
    return;
  double al[K - 1];
#pragma unroll
  for (int j = 0; j < K - 1; ++j)
    al[j] = j < m ? alpha_hist[lo + j] : 0.0;
  const int64_t n2 = n >> 1;
  dbl2* __restrict__ x2 = reinterpret_cast<dbl2*>(x);
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * VB)
  {
    dbl2 xi = x2[i];
#pragma unroll
    for (int j = 0; j < K - 1; ++j)
      if (j < m)
      {
        const dbl2 pj = reinterpret_cast<const dbl2*>(ring.slot[j])[i];
        xi.x = al[j] * pj.x + xi.x;
        xi.y = al[j] * pj.y + xi.y;
      }
    x2[i] = xi;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    double xi = x[n - 1];
#pragma unroll
    for (int j = 0; j < K - 1; ++j)
      if (j < m)
        xi = al[j] * ring.slot[j][n - 1] + xi;
    x[n - 1] = xi;
  }
}

typedef void (*update_p_ring_fn)(CgState*, double*, double*, const double*, int, CgParams, const double*, const double*, int,
                                 const double*, const double*, double*, PRing, double*, int64_t, int, DinvCodes);
template <bool NT, int DZ>
static update_p_ring_fn pick_update_p_flush(int K)
{
  return K == 2 ? k_update_p_flush<NT, DZ, 2> : K == 4 ? k_update_p_flush<NT, DZ, 4> : k_update_p_flush<NT, DZ, 8>;
}

template <bool NT, int DZ = 0>
__global__ __launch_bounds__(VB) void k_update_xr(CgState* __restrict__ st, const double* __restrict__ beta_hist,
                                                  double* __restrict__ alpha_hist, int it,
                                                  const double* __restrict__ pw_parts, int npw,
                                                  const double* __restrict__ w, const double* __restrict__ dinv,
                                                  double* __restrict__ r, double* __restrict__ z, int64_t n, int norm,
                                                  double* __restrict__ pa, double* __restrict__ pb, int variant,
                                                  DinvCodes dz = DinvCodes())
{
  __shared__ double dtab[dz_table(DZ)];
  dz_stage<DZ>(dtab, dz);
  // first entries requested before the scalar prologue (see k_update_p)
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * VB;
  const int64_t i0 = blockIdx.x * (int64_t)VB + threadIdx.x;
  const dbl2* __restrict__ w2 = reinterpret_cast<const dbl2*>(w);
  const dbl2* __restrict__ d2 = reinterpret_cast<const dbl2*>(dinv);
  dbl2* __restrict__ r2 = reinterpret_cast<dbl2*>(r);
  dbl2* __restrict__ z2 = reinterpret_cast<dbl2*>(z);
  const int64_t c0 = (i0 < n2) ? i0 : 0;
  dbl2 wi0 = {0, 0}, di0 = {0, 0}, ri0 = {0, 0};
  uint32_t dc0 = 0;
  // (the scalar inputs of the prologue are requested in the same breath, below: flag, beta, <p,w>)
  if (n2 > 0)
  {
    wi0 = vload<NT>(w2 + c0); // last use of w
    if (DZ)
      dc0 = dz_load2<DZ>(dz, c0);
    else
      di0 = vload<NT>(d2 + c0);
    ri0 = vload<NT>(r2 + c0); // r and D^-1 are touched once per iteration
  }
  const int f0 = st->converged;
  const double beta_it = beta_hist[it];
  const double pw1 = pw_parts[0]; // the all-reduced value itself when a communicator is attached (npw == 1)
  if (block_flag(f0))
    return;
  __shared__ double sh[VB / 64];
  const double pw = npw == 1 ? pw1 : reduce_parts_bcast(pw_parts, npw, sh);
  const double alpha = beta_it / pw; // src/cg.h:65
  // KSPCG stops on a non-finite scalar (KSP_DIVERGED_NANORINF / _BREAKDOWN); linalg::cg has no such guard: with
  // rnorm0 == 0 its alpha is 0/0, every comparison with NaN is false and the loop runs kmax times (src/cg.h:58-83)
  if (variant != ZZZ_CG_CGH && !isfinite(alpha))
  {
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
      st->iters = it;
      st->converged = 2;
      __atomic_store_n(&st->conv_it1, it + 1, __ATOMIC_RELAXED);
    }
    return; // every workgroup sees the same non-finite alpha
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    alpha_hist[it] = alpha; // x += alpha p: applied by k_update_p(it + 1)
  double sa = 0, sb = 0;
  for (int64_t i = i0; i < n2; i += stride)
  {
    dbl2 wi, di, ri, zi;
    if (i == i0)
    {
      wi = wi0;
      di = di0;
      ri = ri0;
    }
    else
    {
      wi = vload<NT>(w2 + i);
      if (!DZ)
        di = vload<NT>(d2 + i);
      ri = vload<NT>(r2 + i);
    }
    if (DZ)
    {
      const uint32_t dc = i == i0 ? dc0 : dz_load2<DZ>(dz, i);
      di.x = dtab[dz_lo<DZ>(dc)];
      di.y = dtab[dz_hi<DZ>(dc)];
    }
    ri.x = -alpha * wi.x + ri.x; // src/cg.h:71
    ri.y = -alpha * wi.y + ri.y;
    zi.x = di.x * ri.x;
    zi.y = di.y * ri.y;
    if (DZ)
      r2[i] = ri; // (read again by k_update_p: left in the cache)
    else
    {
      vstore<NT>(ri, r2 + i);
      z2[i] = zi;
    }
    sa += ri.x * zi.x;
    sa += ri.y * zi.y;
    if (norm == ZZZ_NORM_UNPRECONDITIONED)
    {
      sb += ri.x * ri.x;
      sb += ri.y * ri.y;
    }
    else
    {
      sb += zi.x * zi.x;
      sb += zi.y * zi.y;
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    const int64_t i = n - 1;
    const double ri = -alpha * w[i] + r[i];
    const double zi = (DZ ? dtab[dz_load1<DZ>(dz, i)] : dinv[i]) * ri;
    r[i] = ri;
    if (!DZ)
      z[i] = zi;
    sa += ri * zi;
    sb += (norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : zi * zi;
  }
  const double ta = block_reduce_sum(sa, sh);
  const double tb = block_reduce_sum(sb, sh);
  if (threadIdx.x == 0)
  {
    pa[blockIdx.x] = ta;
    pb[blockIdx.x] = tb;
  }
}

// ---- PETSc's -ksp_cg_single_reduction (KSPCGUseSingleReduction; Chronopoulos/Gear form) ----------
// One iteration = this kernel + one SpMV (s = A z with the partials of <z,s>, <r,z> and the norm):
//   b = beta_k/beta_{k-1};  <p,w>_k = <z,s> - beta_k^2 <p,w>_{k-1} / beta_{k-1}^2;  a = beta_k / <p,w>_k
//   p = z + b p;  w = s + b w  (= A p by recurrence);  x += a p;  r -= a w;  z = D^-1 r
// so a whole iteration has ONE reduction point (after the SpMV) instead of two.
// pa/pb/pc: partials (or the single all-reduced values) of <r,z>, the test norm^2 and <z,s>.
// CHEB (Chebyshev-Jacobi preconditioner, cg_solve_single_reduction): z = D^-1 r becomes the polynomial's first term --
// g = D^-1 r, d = g / theta, z = d (k_cheb_xr's tail) -- and its further terms follow as product epilogues.
// DZ (round 5): as in k_update_p -- Jacobi's inverse diagonal as 16-bit codes into a table in LDS, and z = D^-1 r of the
// LAST iteration recomputed from the r this kernel reads anyway (the same product of the same two doubles: the same bits)
// instead of read back: 96 -> 82 B per row and iteration.  z is still written: the product gathers it.
template <bool NT, bool CHEB = false, int DZ = 0>
__global__ __launch_bounds__(VB) void k_sr_update(CgState* __restrict__ st, double* __restrict__ beta_hist,
                                                  double* __restrict__ dpi_hist, double* __restrict__ dp_hist, int it,
                                                  CgParams P, const double* __restrict__ pa, const double* __restrict__ pb,
                                                  const double* __restrict__ pc, int np, const double* __restrict__ dinv,
                                                  const double* __restrict__ s, double* __restrict__ z, double* __restrict__ p,
                                                  double* __restrict__ w, double* __restrict__ x, double* __restrict__ r,
                                                  int64_t n, int scalars_only, double theta = 0.0, double* __restrict__ chg = nullptr,
                                                  double* __restrict__ chd = nullptr, DinvCodes dz = DinvCodes())
{
  static_assert(!(CHEB && DZ), "the polynomial's first term is not D^-1 r alone");
  __shared__ double dtab[dz_table(DZ)];
  dz_stage<DZ>(dtab, dz);
  // first entries requested before the scalar prologue (see k_update_p): seven 16-B loads in flight per thread while
  // the workgroup walks the flag, the three partial sums and the convergence logic
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * VB;
  const int64_t i0 = blockIdx.x * (int64_t)VB + threadIdx.x;
  const dbl2* __restrict__ s2 = reinterpret_cast<const dbl2*>(s);
  const dbl2* __restrict__ d2 = reinterpret_cast<const dbl2*>(dinv);
  dbl2 *__restrict__ z2 = reinterpret_cast<dbl2*>(z), *__restrict__ p2 = reinterpret_cast<dbl2*>(p),
                     *__restrict__ w2 = reinterpret_cast<dbl2*>(w), *__restrict__ x2 = reinterpret_cast<dbl2*>(x),
                     *__restrict__ r2 = reinterpret_cast<dbl2*>(r);
  const int64_t c0 = (i0 < n2) ? i0 : 0;
  dbl2 zi0 = {0, 0}, si0 = {0, 0}, di0 = {0, 0}, xi0 = {0, 0}, ri0 = {0, 0}, po0 = {0, 0}, wo0 = {0, 0};
  uint32_t dc0 = 0;
  if (n2 > 0 && !scalars_only)
  {
    if (DZ)
      dc0 = dz_load2<DZ>(dz, c0);
    else
    {
      zi0 = z2[c0];
      di0 = vload<NT>(d2 + c0);
    }
    si0 = vload<NT>(s2 + c0);
    xi0 = vload<NT>(x2 + c0);
    ri0 = vload<NT>(r2 + c0);
    po0 = vload<NT>(p2 + c0); // zero before the first iteration (cg_solve_single_reduction clears p and w)
    wo0 = vload<NT>(w2 + c0);
  }
  // ... and so are the scalar inputs: flag, tolerances, last iteration's coefficients, and (communicator attached:
  // np == 1) the three all-reduced sums themselves -- that prologue then has no barrier and one memory round trip
  const int f0 = st->converged;
  const double ttol_st = st->ttol, dp0_st = st->dp0;
  const double bo_h = it > 0 ? beta_hist[it - 1] : 1.0, dpi_h = it > 0 ? dpi_hist[it - 1] : 0.0;
  double rz = pa[0], nn = pb[0], zs = pc[0];
  if (np == 1)
  {
    // every thread holds the same flag unless workgroup 0 of THIS launch is just setting it -- and then every
    // workgroup reaches the same verdict from the same scalars and leaves below: no wavefront updates a vector
    if (f0)
      return;
  }
  else
  {
    if (block_flag(f0))
      return;
    reduce_parts3_bcast(pa, pb, pc, np, rz, nn, zs);
  }
  const double dp = (P.norm == ZZZ_NORM_NATURAL) ? sqrt(fabs(rz)) : sqrt(nn);
  double ttol = ttol_st;
  if (it == 0)
    ttol = fmax(P.rtol * dp, P.atol);
  int conv = 0;
  if (!isfinite(dp))
    conv = 2;
  else if (dp <= ttol) // KSPConvergedDefault
    conv = 1;
  else if (dp >= P.dtol * (it == 0 ? dp : dp0_st)) // ... KSP_DIVERGED_DTOL
    conv = 3;
  double b = 0.0, dpi = zs;
  if (it > 0)
  {
    const double bo = bo_h;
    b = rz / bo;
    dpi = zs - rz * rz * dpi_h / (bo * bo);
  }
  const double a = rz / dpi;
  if (!conv && !scalars_only && !isfinite(a))
    conv = 2;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    beta_hist[it] = rz;
    dpi_hist[it] = dpi;
    dp_hist[it] = dp;
    st->dp = dp;
    if (it == 0)
    {
      st->dp0 = dp;
      st->ttol = ttol;
    }
    if (conv)
    {
      st->iters = it;
      st->converged = conv;
    }
  }
  if (conv || scalars_only)
    return;
  auto one = [&](int64_t i) {
    const double dv = DZ ? dtab[dz_load1<DZ>(dz, i)] : dinv[i];
    const double zo = DZ ? dv * r[i] : z[i];
    const double pn = (it == 0) ? zo : b * p[i] + zo;
    const double wn = (it == 0) ? s[i] : b * w[i] + s[i];
    p[i] = pn;
    w[i] = wn;
    x[i] = a * pn + x[i];
    const double ri = -a * wn + r[i];
    r[i] = ri;
    const double zi = dv * ri;
    if (CHEB)
    {
      chg[i] = zi;
      chd[i] = zi / theta;
      z[i] = zi / theta;
    }
    else
      z[i] = zi;
  };
  for (int64_t i = i0; i < n2; i += stride)
  {
    // cache policy: only z (gathered by the next SpMV) and s (its output) are worth keeping; p, w, x, r, D^-1
    // are touched by this kernel alone, once per iteration
    dbl2 zi, si, di, xi, ri, po, wo;
    uint32_t dc = dc0;
    if (i == i0)
    {
      zi = zi0, si = si0, di = di0, xi = xi0, ri = ri0, po = po0, wo = wo0;
    }
    else
    {
      if (DZ)
        dc = dz_load2<DZ>(dz, i);
      else
        zi = z2[i], di = vload<NT>(d2 + i);
      si = vload<NT>(s2 + i), xi = vload<NT>(x2 + i), ri = vload<NT>(r2 + i);
      if (it != 0)
        po = vload<NT>(p2 + i), wo = vload<NT>(w2 + i);
    }
    if (DZ)
    {
      di.x = dtab[dz_lo<DZ>(dc)];
      di.y = dtab[dz_hi<DZ>(dc)];
      zi.x = di.x * ri.x; // z = D^-1 r as the last iteration (or k_init_residual) formed it
      zi.y = di.y * ri.y;
    }
    dbl2 pn = zi, wn = si, zn;
    if (it != 0)
    {
      pn.x = b * po.x + zi.x;
      pn.y = b * po.y + zi.y;
      wn.x = b * wo.x + si.x;
      wn.y = b * wo.y + si.y;
    }
    xi.x = a * pn.x + xi.x;
    xi.y = a * pn.y + xi.y;
    ri.x = -a * wn.x + ri.x;
    ri.y = -a * wn.y + ri.y;
    zn.x = di.x * ri.x;
    zn.y = di.y * ri.y;
    vstore<NT>(pn, p2 + i);
    vstore<NT>(wn, w2 + i);
    vstore<NT>(xi, x2 + i);
    vstore<NT>(ri, r2 + i);
    if (CHEB)
    {
      dbl2 dn;
      dn.x = zn.x / theta;
      dn.y = zn.y / theta;
      reinterpret_cast<dbl2*>(chg)[i] = zn;
      reinterpret_cast<dbl2*>(chd)[i] = dn;
      z2[i] = dn;
    }
    else
      z2[i] = zn;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    one(n - 1);
}

__device__ inline double reduce_parts(const double* __restrict__ parts, int np, double* sh)
{
  double s = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x)
    s += parts[i];
  return block_reduce_sum(s, sh);
}

__global__ __launch_bounds__(VB) void k_sqnorm(const double* __restrict__ v, int64_t n, double* __restrict__ parts)
{
  __shared__ double sh[VB / 64];
  double s = 0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    s += v[i] * v[i];
  const double t = block_reduce_sum(s, sh);
  if (threadIdx.x == 0)
    parts[blockIdx.x] = t;
}
__global__ __launch_bounds__(1024) void k_reduce_plain(const double* __restrict__ parts, int np, double* out)
{
  __shared__ double sh[16];
  const double s = reduce_parts(parts, np, sh);
  if (threadIdx.x == 0)
    out[0] = s;
}

// The inverse diagonal (ctx->dinv, n entries) as 16-bit codes into a table of its distinct values, for the kernels that take
// DinvCodes: dzc.codes stays null when there are more than DZ_MAX values.  Synchronises the stream once (the count).
int dinv_codes_build(zzz_ctx* ctx, int64_t n, DinvCodes& dzc)
{
  hipStream_t s = ctx->stream;
  const int64_t npad = (n + 1) & ~(int64_t)1;
  ValSet<DD_BITS, 0>& vs = ctx->dd_set;
  ZZZ_HIP(ctx, vs.begin(DZ_MAX, s, ctx->retired));
  ZZZ_HIP(ctx, ctx->dd_codes.reserve((size_t)npad));
  const unsigned gd = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_dd_insert, dim3(gd), dim3(256), 0, s, ctx->dinv.p, n, vs.table.p, vs.info.p, DZ_MAX);
  vs.number(s);
  // ZZZ_CG_DINV_CODES=3: 16-bit codes even where 8 would do (the A/B reference of the 8-bit form)
  const int allow8 = ctx->knob.cg_dinv_codes != 3;
  hipLaunchKernelGGL(k_dd_encode, dim3(gd), dim3(256), 0, s, ctx->dinv.p, n, npad, vs.table.p, vs.slot.p, ctx->dd_codes.p, vs.info.p,
                     allow8);
  int nd = 0;
  ZZZ_HIP(ctx, vs.finish(s, nd));
  if (nd)
    dzc = DinvCodes{reinterpret_cast<const uint32_t*>(ctx->dd_codes.p), vs.dict.p, ctx->r.p, nd, (allow8 && nd <= DZ8_MAX) ? 8 : 16};
  return ZZZ_OK;
}

// bytes one CG iteration touches (operator + `nvec` vectors) against the Infinity Cache
bool loop_exceeds_cache(zzz_ctx* ctx, int nvec)
{
  const double op = sellp_active(ctx) ? (double)sellp_stream_bytes(ctx, true) : 10.0 * (double)ctx->nnz;
  return op + 8.0 * nvec * (double)ctx->nloc() > 200.0e6;
}

int vgrid(int64_t n)
{
  // at least 8 entries per thread: every workgroup starts by summing the producer's per-workgroup partials, so for
  // small vectors fewer, longer workgroups are faster (1.25 M rows: 57.8 -> 52.9 us per iteration with 610 instead of
  // 2048 workgroups, 0.5 M rows 40.8 -> 37.0 us; 16 per thread the same, 32 slower); large vectors keep 8 per CU
  constexpr int per = 8;
  int64_t g = (n + VB * per - 1) / (VB * per);
  if (g > VGRID_MAX)
    g = VGRID_MAX;
  if (g < 1)
    g = 1;
  return (int)g;
}

void cg_launch_extract_dinv(zzz_ctx* ctx, int64_t n, int jacobi)
{
  hipLaunchKernelGGL(k_extract_dinv, dim3(vgrid(n)), dim3(VB), 0, ctx->stream, ctx->rowptr.p, ctx->cols.p, ctx->vals.p, ctx->dinv.p, n,
                     jacobi);
}
void cg_launch_init_residual(zzz_ctx* ctx, double* z, int64_t n, int norm, double* pa, double* pb)
{
  hipLaunchKernelGGL(k_init_residual, dim3(vgrid(n)), dim3(VB), 0, ctx->stream, ctx->b.p, (const double*)nullptr, ctx->dinv.p, ctx->r.p,
                     z, n, norm, pa, pb);
}

// sum of squares over the owned entries, all-reduced over ranks when a communicator is attached
int vec_norm_local(zzz_ctx* ctx, const double* v, int64_t n, double* out)
{
  const int g = vgrid(n);
  hipLaunchKernelGGL(k_sqnorm, dim3(g), dim3(VB), 0, ctx->stream, v, n, ctx->part_b.p);
  if (ctx->comm)
  {
    int rc = comm_reduce_allreduce(ctx, nullptr, ctx->part_b.p, nullptr, nullptr, g, 1, ctx->red.p);
    if (rc)
      return rc;
  }
  else
    hipLaunchKernelGGL(k_reduce_plain, dim3(1), dim3(1024), 0, ctx->stream, ctx->part_b.p, g, ctx->red.p);
  ZZZ_HIP(ctx, hipGetLastError());
  double s = 0;
  ZZZ_HIP(ctx, hipMemcpyAsync(&s, ctx->red.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ZZZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = std::sqrt(s);
  return comm_p2p_check(ctx);
}

static int cg_solve_single_reduction(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm);

// How the solve ended, in KSPConvergedReason's numbering [EXT: petscksp.h]: the reference's solver_function returns
// solver.solve()'s iteration count whatever the reason (src/poisson_problem.cpp:172-178) and the driver prints its summary
// and timings all the same, so a diverged solve is NOT an error here either -- unless the caller asks for PETSc's
// -ksp_error_if_not_converged (zzz_solver_opts.error_if_not_converged).
static int finish_reason(zzz_ctx* ctx, const zzz_solver_opts* o, const CgState& fin, int its)
{
  int reason;
  if (fin.converged == 1)
    reason = (o->variant != ZZZ_CG_CGH && fin.dp < o->atol) ? 3 /* KSP_CONVERGED_ATOL */ : 2 /* KSP_CONVERGED_RTOL */;
  else if (fin.converged == 2)
    reason = -9; // KSP_DIVERGED_NANORINF
  else if (fin.converged == 3)
    reason = -4; // KSP_DIVERGED_DTOL
  else
    reason = -3; // KSP_DIVERGED_ITS (linalg::cg, src/cg.h:58-83, simply returns kmax)
  ctx->last_reason = reason;
  if (o->error_if_not_converged && reason < 0)
  {
    if (reason == -9)
      return fail(ctx, ZZZ_ERR_DIVERGED, "KSP_DIVERGED_NANORINF: CG broke down, non-finite scalar at iteration %d", its);
    if (reason == -4)
      return fail(ctx, ZZZ_ERR_DIVERGED, "KSP_DIVERGED_DTOL: norm %g >= divtol x initial norm %g at iteration %d", fin.dp,
                  fin.dp0, its);
    return fail(ctx, ZZZ_ERR_DIVERGED, "KSP_DIVERGED_ITS: %d iterations without reaching the tolerance (norm %g)", its, fin.dp);
  }
  return ZZZ_OK;
}

// What zzz_cg_info reports about a solve, at the values of a solve with nothing special about it: every solve starts
// here (and so does the solve a spectrum estimate belongs to, after the estimate's own short solve)
void cg_report_reset(zzz_ctx* ctx)
{
  ctx->last_pc_bound = 0.0;
  ctx->last_solve_red_overlapped = false;
  ctx->last_solve_xdefer_k = 1;
  ctx->last_solve_dinv_codes = 0;
  ctx->last_solve_dinv_bits = 0;
}

int CgSolve::begin(zzz_ctx* c, const zzz_solver_opts* opts, int prof_stride)
{
  ctx = c;
  o = opts;
  stride = prof_stride;
  ZZZ_HIP(ctx, ctx->beta_hist.reserve((size_t)o->max_it + 2));
  ZZZ_HIP(ctx, ctx->dp_hist.reserve((size_t)o->max_it + 2));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->state.p, 0, sizeof(CgState), ctx->stream));
  // profiling events around the product launches
  max_prof = o->profile ? 512 : 0;
  if ((int)ctx->ev.size() < 2 * max_prof)
  {
    size_t old = ctx->ev.size();
    ctx->ev.resize(2 * max_prof);
    for (size_t i = old; i < ctx->ev.size(); ++i)
      ZZZ_HIP(ctx, hipEventCreate(&ctx->ev[i]));
  }
  ctx->prof_halo_n = 0;
  ctx->prof_halo_wait_ms = 0.0;
  ZZZ_HIP(ctx, chk_ev.create());
  return ZZZ_OK;
}

// An event record between two kernels is not free (PROF_STRIDE, zzz_cg.h): only every stride-th product is timed.
// prof_now lets the halo exchange of a timed product sample its exposed wait (zzz_comm.hip).
void CgSolve::product_begin(int it)
{
  timed = nprof < max_prof && it % stride == 0;
  ctx->prof_now = timed;
  if (timed)
    (void)hipEventRecord(ctx->ev[2 * nprof], ctx->stream);
}

int CgSolve::product_end(int rc)
{
  ctx->prof_now = false;
  if (rc)
    return rc;
  if (timed)
  {
    (void)hipEventRecord(ctx->ev[2 * nprof + 1], ctx->stream);
    ++nprof;
  }
  return ZZZ_OK;
}

int CgSolve::poll(int done)
{
  if (done % CHECK != 0)
    return ZZZ_OK;
  const int slot = nchk % NSLOT;
  if (nchk >= NSLOT - 1)
  {
    const int old = (nchk - (NSLOT - 1)) % NSLOT;
    ZZZ_HIP(ctx, hipEventSynchronize(chk_ev[old]));
    if (ctx->h_state[old].converged)
      stop = true;
  }
  ZZZ_HIP(ctx, hipMemcpyAsync(&ctx->h_state[slot], ctx->state.p, sizeof(CgState), hipMemcpyDeviceToHost, ctx->stream));
  ZZZ_HIP(ctx, hipEventRecord(chk_ev[slot], ctx->stream));
  ++nchk;
  return ZZZ_OK;
}

int CgSolve::finish(int* iters, double* rnorm)
{
  hipStream_t s = ctx->stream;
  ZZZ_HIP(ctx, hipGetLastError());
  CgState fin;
  ZZZ_HIP(ctx, hipMemcpyAsync(&fin, ctx->state.p, sizeof(CgState), hipMemcpyDeviceToHost, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s));
  if (int rc = comm_p2p_check(ctx)) // (nothing without a communicator)
    return rc;

  const int its = fin.converged ? fin.iters : o->max_it;
  ctx->last_iters = its;
  if (iters)
    *iters = its;
  if (rnorm)
  {
    rnorm[0] = fin.dp;
    rnorm[1] = fin.dp0;
  }
  ctx->history.resize((size_t)its + 1);
  ZZZ_HIP(ctx, hipMemcpy(ctx->history.data(), ctx->dp_hist.p, sizeof(double) * ((size_t)its + 1), hipMemcpyDeviceToHost));

  ctx->prof_spmv_ms = 0.0;
  ctx->prof_spmv_n = 0;
  const int used = std::min(nprof, (its + stride - 1) / stride); // launches past convergence return at once: not counted
  for (int i = 0; i < used; ++i)
  {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]) == hipSuccess)
    {
      ctx->prof_spmv_ms += ms;
      ctx->prof_spmv_n++;
    }
  }
  if (ctx->prof_spmv_n)
    ctx->prof_spmv_ms /= (double)ctx->prof_spmv_n;
  // the exposed halo wait, over the samples comm_halo_forward took while prof_now was set
  int cnt = 0;
  for (int i = 0; i < ctx->prof_halo_n; ++i)
  {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_halo[(size_t)(2 * i)], ctx->ev_halo[(size_t)(2 * i + 1)]) == hipSuccess)
    {
      ctx->prof_halo_wait_ms += ms;
      ++cnt;
    }
  }
  if (cnt)
    ctx->prof_halo_wait_ms /= cnt;
  (void)hipGetLastError();
  return finish_reason(ctx, o, fin, its);
}

static int cg_solve_pc(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm);

int cg_solve(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm)
{
  cg_report_reset(ctx);
  if (int rc = comm_inproc_meet(ctx))
    return rc;
  if (o->variant == ZZZ_CG_PIPE)
    return cg_solve_pipe(ctx, o, iters, rnorm); // zzz_cg_pipe.hip
  if ((o->pc == ZZZ_PC_CHEBYSHEV_JACOBI && !o->single_reduction) || o->pc == ZZZ_PC_MG || o->pc == ZZZ_PC_PMG || o->pc == ZZZ_PC_AGG
      || o->pc == ZZZ_PC_SAGG || o->pc == ZZZ_PC_SAGG_RBM)
    return cg_solve_pc(ctx, o, iters, rnorm);
  if (o->single_reduction)
    return cg_solve_single_reduction(ctx, o, iters, rnorm);
  const int64_t n = ctx->n_owned * ctx->bs; // owned scalar rows
  const int max_it = o->max_it;
  CgParams P{o->variant, o->pc, o->norm, o->rtol, o->atol, o->dtol > 0.0 ? o->dtol : 1.0e4};
  const bool multi = ctx->comm != nullptr;
  const int g = vgrid(n);
  hipStream_t s = ctx->stream;
  const bool nt = loop_exceeds_cache(ctx, 6);
  // (kernels by load policy and by the form of the inverse diagonal: chosen below, where dzc is known)

  CgSolve S;
  if (int rc = S.begin(ctx, o))
    return rc;
  ZZZ_HIP(ctx, ctx->alpha_hist.reserve((size_t)max_it + 2));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->p.p, 0, sizeof(double) * ctx->p.n, s));

  // PCSetUp(PCJACOBI): inverse diagonal (inside `ZZZ Solve`, as KSPSetUp is in the reference)
  if (o->op == ZZZ_OP_CSR)
    hipLaunchKernelGGL(k_extract_dinv, dim3(g), dim3(VB), 0, s, ctx->rowptr.p, ctx->cols.p, ctx->vals.p, ctx->dinv.p, n,
                       o->pc == ZZZ_PC_JACOBI ? 1 : 0);
  else if (o->pc == ZZZ_PC_JACOBI)
  {
    // the operator is never assembled: its diagonal from the element matrices (zzz_matfree.hip), inverted in place
    if (int rc = launch_matfree_diagonal(ctx, ctx->dinv.p))
      return rc;
    hipLaunchKernelGGL(k_invert, dim3(g), dim3(VB), 0, s, ctx->dinv.p, n);
  }
  else
    hipLaunchKernelGGL(k_extract_dinv, dim3(g), dim3(VB), 0, s, (const rp_t*)nullptr, (const int32_t*)nullptr,
                       (const double*)nullptr, ctx->dinv.p, n, 0);

  // Jacobi's inverse diagonal as 16-bit codes and no z vector (DinvCodes, k_update_p): KSPCG + PCJACOBI, a loop too large for
  // the Infinity Cache (where bytes are what the vector kernels wait for: the criterion of their load policy;
  // ZZZ_CG_DINV_CODES: 0 never, 2 at any size), at most 2 048 values
  DinvCodes dzc{nullptr, nullptr, nullptr, 0, 0};
  if (o->variant == ZZZ_CG_PETSC && o->pc == ZZZ_PC_JACOBI && ctx->knob.cg_dinv_codes != 0 && (ctx->knob.cg_dinv_codes >= 2 || nt))
    if (int rc = dinv_codes_build(ctx, n, dzc))
      return rc;
  ctx->last_solve_dinv_codes = dzc.codes ? dzc.ndict : 0;
  ctx->last_solve_dinv_bits = dzc.codes ? dzc.bits : 0;
  const int form = dz_form(dzc);
  auto kern_update_p = dz_dispatch(nt, form, [](auto NT, auto DZ) { return k_update_p<decltype(NT)::value, decltype(DZ)::value>; });
  auto kern_update_xr = dz_dispatch(nt, form, [](auto NT, auto DZ) { return k_update_xr<decltype(NT)::value, decltype(DZ)::value>; });

  // The solution update deferred (k_update_p_light / _flush): where x comes from HBM, i.e. under the same rule as the
  // load policy (ZZZ_CG_XDEFER: 0 never, 2 at any size; ZZZ_CG_XDEFER_K: the ring's length).  Slot 0 is ctx->p, the other
  // slots are allocated at the first solve that uses them and kept.  Owned entries of a slot are written in full by the
  // k_update_p that forms its direction before anything reads them; ghost tail and padding are cleared here, once per solve,
  // as the memset above does for ctx->p.
  int K = (ctx->knob.cg_xdefer != 0 && (ctx->knob.cg_xdefer == 2 || nt)) ? ctx->knob.cg_xdefer_k : 1;
  PRing ring{};
  ring.slot[0] = ctx->p.p;
  for (int j = 1; j < K; ++j)
  {
    DevBuf<double>& rb = ctx->p_ring[j - 1];
    const double* before = rb.p;
    if (rb.reserve(ctx->p.n) != hipSuccess)
    {
      (void)hipGetLastError();
      for (DevBuf<double>& b : ctx->p_ring)
        b.release();
      fprintf(stderr, "zzz: no memory for %d more direction vectors of %zu entries: CG updates the solution in every iteration (K = 1)\n",
              K - 1, ctx->p.n);
      K = 1;
      break;
    }
    if (rb.p != before)
      ZZZ_HIP(ctx, hipMemsetAsync(rb.p, 0, sizeof(double) * rb.cap, s));
    else if (ctx->p.n > (size_t)n)
      ZZZ_HIP(ctx, hipMemsetAsync(rb.p + n, 0, sizeof(double) * (ctx->p.n - (size_t)n), s));
    ring.slot[j] = rb.p;
  }
  ctx->last_solve_xdefer_k = K;
  update_p_ring_fn kern_light = nullptr, kern_flush = nullptr;
  if (K > 1)
  {
    kern_light = dz_dispatch(nt, form, [](auto NT, auto DZ) { return k_update_p_light<decltype(NT)::value, decltype(DZ)::value>; });
    kern_flush = dz_dispatch(nt, form, [K](auto NT, auto DZ) { return pick_update_p_flush<decltype(NT)::value, decltype(DZ)::value>(K); });
  }
  // the test of iteration k and (update_dir) the direction p_k; where p_k lives
  auto dir_of = [&](int k) { return ring.slot[k % K]; };
  auto launch_update_p = [&](int k, int update_dir, const double* rz_src, const double* nn_src, int n_rz) {
    if (K == 1)
      hipLaunchKernelGGL(kern_update_p, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->dp_hist.p, ctx->alpha_hist.p, k,
                         P, rz_src, nn_src, n_rz, ctx->z.p, ctx->p.p, ctx->u.p, n, update_dir, dzc);
    else
      hipLaunchKernelGGL((k > 0 && k % K == 0) ? kern_flush : kern_light, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p,
                         ctx->dp_hist.p, ctx->alpha_hist.p, k, P, rz_src, nn_src, n_rz, ctx->z.p, (const double*)dir_of(k + K - 1),
                         dir_of(k), ring, ctx->u.p, n, update_dir, dzc);
  };

  auto apply = [&](double* x, double* y, double* parts, int* np) -> int {
    if (o->op == ZZZ_OP_CSR)
      return launch_product(ctx, x, y, parts, np);
    if (multi)
      if (int rc = comm_halo_forward(ctx, x))
        return rc;
    return launch_matfree_action(ctx, x, y, parts, np);
  };

  // initial residual
  const double* w0 = nullptr;
  if (o->variant == ZZZ_CG_CGH)
  {
    int rc = apply(ctx->u.p, ctx->w.p, nullptr, nullptr); // action(x, y), src/cg.h:46
    if (rc)
      return rc;
    w0 = ctx->w.p;
  }
  else
    ZZZ_HIP(ctx, hipMemsetAsync(ctx->u.p, 0, sizeof(double) * ctx->u.n, s)); // KSP zero initial guess
  double* pa = ctx->part_b.p;
  double* pb = ctx->part_b.p + VGRID_MAX;
  // (the matrix-free operator is served by this loop alone: every other form asks for the assembled one)
  const bool lifted_mf = o->op == ZZZ_OP_MATFREE && ctx->dirichlet.have_bc_val;
  const double* rhs = ctx->b.p;
  if (lifted_mf)
  {
    ZZZ_HIP(ctx, ctx->b_masked.grow_keep((size_t)n, ctx->retired));
    hipLaunchKernelGGL(k_masked_copy, dim3(g), dim3(VB), 0, s, ctx->b.p, ctx->bc.p, ctx->b_masked.p, n);
    rhs = ctx->b_masked.p;
  }
  hipLaunchKernelGGL(k_init_residual, dim3(g), dim3(VB), 0, s, rhs, w0, ctx->dinv.p, ctx->r.p, ctx->z.p, n, P.norm,
                     pa, pb);
  // where the consumer kernels find <r,z>, the test norm and <p,w>: the producers' partials, or the
  // single all-reduced value when a communicator is attached
  const double *rz_src = pa, *nn_src = pb, *pw_src = ctx->part_a.p;
  int n_rz = g;
  if (multi)
  {
    rz_src = ctx->red.p;
    nn_src = ctx->red.p + 1;
    pw_src = ctx->red.p + 2;
    n_rz = 1;
  }
  const int* stop_flag = reinterpret_cast<const int*>(ctx->state.p); // CgState::converged
  auto allreduce_beta = [&]() -> int {
    if (!multi)
      return ZZZ_OK;
    return comm_reduce_allreduce(ctx, stop_flag, pa, pb, nullptr, g, 2, ctx->red.p);
  };
  {
    int rc = allreduce_beta();
    if (rc)
      return rc;
  }

  int it = 0;
  for (; it < max_it && !S.stop; ++it)
  {
    // convergence test of iteration `it` and the new search direction
    launch_update_p(it, 1, rz_src, nn_src, n_rz);
    int np = 0;
    S.product_begin(it);
    if (int rc = S.product_end(apply(dir_of(it), ctx->w.p, ctx->part_a.p, &np)))
      return rc;
    if (multi)
    {
      int rc = comm_reduce_allreduce(ctx, stop_flag, ctx->part_a.p, nullptr, nullptr, np, 1, ctx->red.p + 2);
      if (rc)
        return rc;
      np = 1;
    }
    hipLaunchKernelGGL(kern_update_xr, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->alpha_hist.p, it, pw_src,
                       np, ctx->w.p, ctx->dinv.p, ctx->r.p, ctx->z.p, n, P.norm, pa, pb, P.variant, dzc);
    if (int rc = allreduce_beta())
      return rc;
    if (int rc = S.poll(it + 1))
      return rc;
  }
  // the test of the last completed iteration (it == max_it when the loop ran out) and its pending
  // solution update; no new direction
  launch_update_p(it, 0, rz_src, nn_src, n_rz);
  // ... and, with the update deferred, those of the iterations since the last flush that ran
  if (K == 2)
    hipLaunchKernelGGL(k_x_apply_pending<2>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->alpha_hist.p, it, ring, ctx->u.p, n);
  else if (K == 4)
    hipLaunchKernelGGL(k_x_apply_pending<4>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->alpha_hist.p, it, ring, ctx->u.p, n);
  else if (K == 8)
    hipLaunchKernelGGL(k_x_apply_pending<8>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->alpha_hist.p, it, ring, ctx->u.p, n);
  if (lifted_mf && o->variant == ZZZ_CG_PETSC) // (src/cg.h leaves u[bc] at the caller's initial guess, and so does ZZZ_CG_CGH)
    hipLaunchKernelGGL(k_set_bc_values, dim3(g), dim3(VB), 0, s, ctx->bc.p, ctx->bc_val.p, ctx->u.p, n);
  return S.finish(iters, rnorm);
}

// ---- KSPCG with the Chebyshev-Jacobi polynomial preconditioner (ZZZ_PC_CHEBYSHEV_JACOBI; oracle: zo_pcg_cheb) -------
// z = p_k(D^-1 A) D^-1 r by k steps of the Chebyshev iteration for D^-1 A on [hi / ratio, hi], hi = Gershgorin's bound:
// no reduction inside the application, k more products per CG iteration, roughly k + 1 times fewer CG iterations and
// all-reduces.  The rest of the iteration is the classical loop's: k_update_p (test, x and p), the product, then k_cheb_xr
// (k_update_xr's r -= alpha w with the polynomial's first term) and one product + k_cheb_step per further term; the last
// k_cheb_step sums <r,z> and the norm.
// The polynomial itself (ChebPlan, cheb_first, cheb_terms: zzz_cg.h) is also the smoother of every multigrid level
// (zzz_mg.hip): one first-term kernel, one further-term kernel, one host recurrence.  The driver cg_solve_pc further down
// is KSPCG around a preconditioner object and serves this preconditioner and the multigrid ones.
__global__ __launch_bounds__(VB) void k_row_abs_max(const rp_t* __restrict__ rowptr, const double* __restrict__ vals,
                                                    const double* __restrict__ dinv, int64_t n, double* __restrict__ parts)
{
  __shared__ double sh[VB / 64];
  double m = 0.0;
  for (int64_t r = blockIdx.x * (int64_t)VB + threadIdx.x; r < n; r += (int64_t)gridDim.x * VB)
  {
    double sum = 0.0;
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
      sum += fabs(vals[k]);
    m = fmax(m, sum * fabs(dinv[r]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    m = fmax(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0)
    sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    for (int i = 1; i < VB / 64; ++i)
      m = fmax(m, sh[i]);
    parts[blockIdx.x] = m;
  }
}
// The polynomial's first term: g = D^-1 (b - t), d = g / theta, x = (x +) d.  t == null: the start from zero, whose
// residual is b and costs no product (the preconditioner; a level's pre-smoother); t = A x: the start from x (the
// post-smoother).
__global__ __launch_bounds__(VB) void k_cheb_first(const int* __restrict__ stop, const double* __restrict__ b,
                                                   const double* __restrict__ t, const double* __restrict__ dinv, double theta,
                                                   double* __restrict__ gv, double* __restrict__ d, double* __restrict__ x, int64_t n)
{
  if (stop && *stop)
    return;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    const double gi = t ? dinv[i] * (b[i] - t[i]) : dinv[i] * b[i];
    const double di = gi / theta;
    gv[i] = gi;
    d[i] = di;
    x[i] = t ? x[i] + di : di;
  }
}
// k_update_xr and k_cheb_first from zero in one pass: alpha = beta / <p,w>; r -= alpha w; g = D^-1 r; d = g / theta; z = d
__global__ __launch_bounds__(VB) void k_cheb_xr(CgState* __restrict__ st, const double* __restrict__ beta_hist,
                                                double* __restrict__ alpha_hist, int it, const double* __restrict__ pw_parts,
                                                int npw, const double* __restrict__ w, const double* __restrict__ dinv,
                                                double theta, double* __restrict__ r, double* __restrict__ gv,
                                                double* __restrict__ d, double* __restrict__ z, int64_t n)
{
  const int f0 = st->converged;
  const double beta_it = beta_hist[it];
  const double pw1 = pw_parts[0];
  if (block_flag(f0))
    return;
  __shared__ double sh[VB / 64];
  const double pw = npw == 1 ? pw1 : reduce_parts_bcast(pw_parts, npw, sh);
  const double alpha = beta_it / pw;
  if (!isfinite(alpha)) // KSP_DIVERGED_NANORINF, as in k_update_xr
  {
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
      st->iters = it;
      st->converged = 2;
      __atomic_store_n(&st->conv_it1, it + 1, __ATOMIC_RELAXED);
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    alpha_hist[it] = alpha;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    const double ri = -alpha * w[i] + r[i];
    const double gi = dinv[i] * ri;
    const double di = gi / theta;
    r[i] = ri;
    gv[i] = gi;
    d[i] = di;
    z[i] = di;
  }
}
// one term of the polynomial, w = A d_(j-1) given: g -= D^-1 w; d_j = c1 d_(j-1) + c2 g; z += d_j.  The last term leaves
// g and d alone and sums the partials of <r,z> and of the test norm (the arrays k_update_p reads).
__global__ __launch_bounds__(VB) void k_cheb_step(const int* __restrict__ stop, const double* __restrict__ w,
                                                  const double* __restrict__ dinv, double c1, double c2, int last,
                                                  double* __restrict__ gv, double* __restrict__ d, double* __restrict__ z,
                                                  const double* __restrict__ r, int norm, double* __restrict__ pa,
                                                  double* __restrict__ pb, int64_t n)
{
  if (stop && *stop)
    return;
  __shared__ double sh[VB / 64];
  double sa = 0, sb = 0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    double gi, dn;
    cheb_term(dinv[i], w[i], gv[i], d[i], c1, c2, gi, dn);
    const double zi = z[i] + dn;
    z[i] = zi;
    if (!last)
    {
      gv[i] = gi;
      d[i] = dn;
    }
    else
    {
      const double ri = r[i];
      sa += ri * zi;
      sb += (norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : zi * zi;
    }
  }
  if (last)
  {
    const double ta = block_reduce_sum(sa, sh);
    const double tb = block_reduce_sum(sb, sh);
    if (threadIdx.x == 0)
    {
      pa[blockIdx.x] = ta;
      pb[blockIdx.x] = tb;
    }
  }
}
// partials of <r,z> and of the test norm (the arrays k_update_p reads)
__global__ __launch_bounds__(VB) void k_dots_rz(const int* __restrict__ stop, const double* __restrict__ r,
                                                const double* __restrict__ z, int64_t n, int norm, double* __restrict__ pa,
                                                double* __restrict__ pb)
{
  if (*stop)
    return;
  __shared__ double sh[VB / 64];
  double sa = 0, sb = 0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    const double ri = r[i], zi = z[i];
    sa += ri * zi;
    sb += (norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : zi * zi;
  }
  const double ta = block_reduce_sum(sa, sh);
  const double tb = block_reduce_sum(sb, sh);
  if (threadIdx.x == 0)
  {
    pa[blockIdx.x] = ta;
    pb[blockIdx.x] = tb;
  }
}

// the noise vector of the spectrum estimate (oracle: zo_noise): a fixed hash of the GLOBAL row number in the caller's
// numbering, so that neither the library's internal order nor the partition changes the estimate
__global__ __launch_bounds__(VB) void k_noise(const int32_t* __restrict__ perm, int bs, int64_t offset, int64_t n,
                                              double* __restrict__ v)
{
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    int64_t row = i;
    if (perm)
      row = (int64_t)perm[i / bs] * bs + i % bs;
    unsigned int h = (unsigned int)((unsigned long long)(offset + row) * 2654435761ull + 12345ull);
    h ^= h >> 16;
    h *= 0x45d9f3bu;
    h ^= h >> 16;
    v[i] = (double)h / 4294967296.0 - 0.5;
  }
}

// largest eigenvalue of the k x k symmetric tridiagonal (diagonal t, off-diagonal e): bisection on the Sturm count
static double tridiag_lmax(int k, const double* t, const double* e)
{
  double lo = t[0], hi = t[0];
  for (int j = 0; j < k; ++j)
  {
    const double rad = (j > 0 ? std::fabs(e[j - 1]) : 0.0) + (j + 1 < k ? std::fabs(e[j]) : 0.0);
    lo = std::min(lo, t[j] - rad);
    hi = std::max(hi, t[j] + rad);
  }
  for (int itb = 0; itb < 200 && hi - lo > 4.0e-16 * std::fabs(hi); ++itb)
  {
    const double mid = 0.5 * (lo + hi);
    int above = 0;
    double q = 1.0;
    for (int j = 0; j < k; ++j)
    {
      const double off2 = j > 0 ? e[j - 1] * e[j - 1] : 0.0;
      q = (t[j] - mid) - (j > 0 ? off2 / q : 0.0);
      if (q == 0.0)
        q = 1.0e-300;
      if (q > 0.0)
        ++above;
    }
    if (above > 0)
      lo = mid;
    else
      hi = mid;
  }
  return 0.5 * (lo + hi);
}

// PETSc's -ksp_chebyshev_esteig: `its` iterations of Jacobi-PCG (the classical loop above, communicator and all) on the
// noise vector; the Lanczos tridiagonal of its step lengths and <r,z> values gives the largest Ritz value of D^-1 A
// (from below: 0.97-0.98 of the eigenvalue after 10 iterations).  0 when it could not be formed.
static int chebyshev_esteig(zzz_ctx* ctx, const zzz_solver_opts* o, int its, double* ritz)
{
  *ritz = 0.0;
  its = std::min(its, 64);
  const int64_t n = ctx->n_owned * ctx->bs;
  int nranks = 1;
  const int me = comm_rank_of(ctx, &nranks);
  std::vector<double> sizes((size_t)nranks);
  if (int rc = comm_allgather_double(ctx, (double)n, sizes.data()))
    return rc;
  int64_t offset = 0;
  for (int r = 0; r < me; ++r)
    offset += (int64_t)sizes[(size_t)r];
  ZZZ_HIP(ctx, ctx->cheb_noise.alloc(ctx->b.n));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->cheb_noise.p, 0, sizeof(double) * ctx->cheb_noise.n, ctx->stream));
  hipLaunchKernelGGL(k_noise, dim3(vgrid(n)), dim3(VB), 0, ctx->stream, ctx->dofmap.renumbered ? ctx->perm.p : (const int32_t*)nullptr,
                     ctx->bs, offset, n, ctx->cheb_noise.p);
  zzz_solver_opts o2 = *o;
  o2.pc = ZZZ_PC_JACOBI;
  o2.norm = ZZZ_NORM_PRECONDITIONED;
  o2.max_it = its;
  o2.rtol = 0.0;
  o2.atol = 0.0;
  o2.dtol = 1.0e300;
  o2.profile = 0;
  o2.single_reduction = 0;
  o2.error_if_not_converged = 0;
  auto swap_b = [&]() {
    std::swap(ctx->b.p, ctx->cheb_noise.p);
    std::swap(ctx->b.n, ctx->cheb_noise.n);
    std::swap(ctx->b.cap, ctx->cheb_noise.cap);
  };
  swap_b();
  int ran = 0;
  double rn[2];
  const int rc = cg_solve(ctx, &o2, &ran, rn);
  swap_b();
  cg_report_reset(ctx); // (zzz_cg_info reports the solve this estimate belongs to, and that one keeps its own kernels)
  if (rc)
    return rc;
  if (ran < 2)
    return ZZZ_OK;
  std::vector<double> alpha((size_t)ran), rho((size_t)ran + 1);
  ZZZ_HIP(ctx, hipMemcpy(alpha.data(), ctx->alpha_hist.p, sizeof(double) * (size_t)ran, hipMemcpyDeviceToHost));
  ZZZ_HIP(ctx, hipMemcpy(rho.data(), ctx->beta_hist.p, sizeof(double) * ((size_t)ran + 1), hipMemcpyDeviceToHost));
  std::vector<double> t((size_t)ran), e((size_t)ran);
  for (int j = 0; j < ran; ++j)
  {
    if (!(alpha[(size_t)j] > 0.0) || !std::isfinite(alpha[(size_t)j]) || !(rho[(size_t)j] > 0.0) || !std::isfinite(rho[(size_t)j]))
      return ZZZ_OK;
    t[(size_t)j] = 1.0 / alpha[(size_t)j] + (j > 0 ? (rho[(size_t)j] / rho[(size_t)j - 1]) / alpha[(size_t)j - 1] : 0.0);
    if (j + 1 < ran)
      e[(size_t)j] = std::sqrt(rho[(size_t)j + 1] / rho[(size_t)j]) / alpha[(size_t)j];
  }
  for (int j = 0; j + 1 < ran; ++j)
    if (!std::isfinite(e[(size_t)j]))
      return ZZZ_OK;
  *ritz = tridiag_lmax(ran, t.data(), e.data());
  return ZZZ_OK;
}

// Spectrum bound (Gershgorin, tightened by the Lanczos estimate; cached per set of matrix values), constants, buffers.
// Runs the estimate's short Jacobi solve through the classical loop: call it BEFORE the caller initialises its own solve.
// Leaves ctx->dinv = 1 / diag(A).
int chebyshev_setup(zzz_ctx* ctx, const zzz_solver_opts* o, ChebPlan& C)
{
  const int64_t n = ctx->n_owned * ctx->bs;
  const bool multi = ctx->comm != nullptr;
  const int g = vgrid(n);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_extract_dinv, dim3(g), dim3(VB), 0, s, ctx->rowptr.p, ctx->cols.p, ctx->vals.p, ctx->dinv.p, n, 1);
  const zzz_ctx::ChebKey key{ctx->mat_version, o->pc_esteig_its == 0 ? 10 : o->pc_esteig_its};
  double hi = 0.0;
  // the bound belongs to the matrix, not to the solve: kept until the values change (every rank sees the same sequence of
  // assemblies and uploads, so all of them take or skip the estimate's collectives together)
  if (ctx->cheb_key == key)
    hi = ctx->cheb_hi;
  else
  {
  // spectrum bound: Gershgorin's for D^-1 A, maximum over the ranks
  hipLaunchKernelGGL(k_row_abs_max, dim3(g), dim3(VB), 0, s, ctx->rowptr.p, ctx->vals.p, ctx->dinv.p, n, ctx->part_b.p);
  std::vector<double> hp((size_t)g);
  ZZZ_HIP(ctx, hipMemcpyAsync(hp.data(), ctx->part_b.p, sizeof(double) * (size_t)g, hipMemcpyDeviceToHost, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s));
  for (double v : hp)
    hi = std::max(hi, v);
  if (multi)
    if (int rc = comm_allgather_max(ctx, &hi))
      return rc;
  if (!(hi > 0.0) || !std::isfinite(hi))
    hi = 1.0;
  // ... tightened by the Lanczos estimate where that is lower (Gershgorin's bound is exact for P1 Laplacians, 2, and up to
  // 2.7 x too high for P2 / P3 / elasticity, which costs 1.6 x the products); safety factor 1.1 as in PETSc
  if (key.est_its > 0)
  {
    double ritz = 0.0;
    if (int rc = chebyshev_esteig(ctx, o, key.est_its, &ritz))
      return rc;
    if (ritz > 0.0 && std::isfinite(ritz) && 1.1 * ritz < hi)
      hi = 1.1 * ritz;
  }
  ctx->cheb_hi = hi;
  ctx->cheb_key = key;
  }
  C = ChebPlan(hi, o->pc_ratio > 1.0 ? o->pc_ratio : 60.0, o->pc_degree > 0 ? o->pc_degree : 3);
  // On the operator stream a term is the EPILOGUE of its product (ChebEpi, zzz_sellp.hip): w = A d never travels through
  // memory and the term costs no launch of its own; d then alternates between two buffers (other lanes still gather the
  // old one).  A/B knob ZZZ_CHEB_FUSED=0: product and k_cheb_step as two launches (the tile kernel's form) -- same bits.
  C.fused = sellp_active(ctx);
  if (const char* e = getenv("ZZZ_CHEB_FUSED"))
    C.fused = C.fused && atoi(e) != 0;
  // (the overlapped product of a partition without a group split is the tile kernel's, launch_product: no epilogue there)
  if (multi && ctx->knob.overlap && ctx->pattern.have_tile_split && !ctx->pattern.have_group_split)
    C.fused = false;
  ZZZ_HIP(ctx, ctx->cheb_d.alloc((size_t)ctx->nloc())); // ghost entries: the product gathers it
  ZZZ_HIP(ctx, ctx->cheb_d2.alloc((size_t)ctx->nloc()));
  ZZZ_HIP(ctx, ctx->cheb_g.alloc((size_t)ctx->nloc()));
  C.d = ctx->cheb_d.p;
  C.d2 = ctx->cheb_d2.p;
  C.g = ctx->cheb_g.p;
  ZZZ_HIP(ctx, hipMemsetAsync(C.d, 0, sizeof(double) * (size_t)ctx->nloc(), s));
  ZZZ_HIP(ctx, hipMemsetAsync(C.d2, 0, sizeof(double) * (size_t)ctx->nloc(), s));
  return ZZZ_OK;
}

void cheb_first(zzz_ctx* c, zzz_ctx* owner, const ChebPlan& C, const double* b, const double* t, double* x)
{
  const int64_t n = c->n_owned * c->bs;
  hipLaunchKernelGGL(k_cheb_first, dim3(vgrid(n)), dim3(VB), 0, owner->stream, reinterpret_cast<const int*>(owner->state.p), b, t,
                     c->dinv.p, C.theta, C.g, C.d, x, n);
}

int cheb_terms(zzz_ctx* c, zzz_ctx* owner, const ChebPlan& C, const double* b, double* x, int norm, double* pa, double* pb, int* np)
{
  const int64_t n = c->n_owned * c->bs;
  const int* stop_flag = reinterpret_cast<const int*>(owner->state.p);
  double rho = 1.0 / C.sigma;
  double *dcur = C.d, *dalt = C.d2;
  for (int st = 1; st < C.degree; ++st)
  {
    const bool last = pa && st + 1 == C.degree;
    double c1, c2;
    C.next_term(rho, c1, c2);
    if (C.fused)
    {
      ChebEpi E;
      E.dinv = c->dinv.p;
      E.g = C.g;
      E.z = x;
      E.r = b;
      E.c1 = c1;
      E.c2 = c2;
      if (int rc = launch_product(c, dcur, dalt, last ? c->part_a.p : nullptr, last ? np : nullptr, nullptr,
                                  norm == ZZZ_NORM_UNPRECONDITIONED ? 1 : 0, &E))
        return rc;
      std::swap(dcur, dalt);
      continue;
    }
    // terms as launches of their own: the product's output goes to the second direction buffer (free in this form; the
    // CG vector w is the single-reduction form's A p and must survive).  (Without a communicator -- every multigrid
    // level -- launch_product is launch_spmv.)
    if (int rc = launch_product(c, dcur, C.d2, nullptr, nullptr))
      return rc;
    hipLaunchKernelGGL(k_cheb_step, dim3(vgrid(n)), dim3(VB), 0, owner->stream, stop_flag, C.d2, c->dinv.p, c1, c2, last ? 1 : 0, C.g,
                       dcur, x, b, norm, pa, pb, n);
  }
  return ZZZ_OK;
}

// ---- KSPCG around a preconditioner object (ZZZ_PC_CHEBYSHEV_JACOBI; ZZZ_PC_MG / _PMG / _AGG / _SAGG / _SAGG_RBM, zzz_mg.hip) ----
// The scalar logic, history and reasons are the classical loop's (k_update_p with Jacobi's semantics for alpha and beta).
// What a preconditioner brings:
struct CgPc
{
  zzz_ctx* ctx;
  const zzz_solver_opts* o;
  int64_t n;
  int g;
  double *pa, *pb; // where k_init_residual, k_update_xr and k_dots_rz leave the partials of <r,z> and of the test norm
  const double *rz, *nn; // where apply left them: pa / pb unless it says otherwise
  int n_rz;
  double bound = 0.0; // zzz_cg_info's spectrum bound
  int prof_stride = PROF_STRIDE;
  // the host reads the state back in EVERY iteration, behind k_update_p and ahead of the product and the application it
  // enqueues before it waits for the copy (one iteration of lag), instead of CgSolve::poll: for an iteration of a few
  // milliseconds of device work, about ten of which make a solve
  bool poll_each = false;
  CgPc(zzz_ctx* c, const zzz_solver_opts* opts)
      : ctx(c), o(opts), n(c->n_owned * c->bs), g(vgrid(n)), pa(c->part_b.p), pb(c->part_b.p + VGRID_MAX), rz(pa), nn(pb), n_rz(g)
  {
  }
  virtual ~CgPc() = default;
  // PCSetUp; sets bound, and prof_stride / poll_each where they differ.  Runs BEFORE CgSolve::begin: it may run solves of
  // its own through the context's CG vectors.
  virtual int setup() = 0;
  // it < 0: z = M r behind k_init_residual (r = b);  else the residual update of iteration `it` (alpha from the npw
  // partials of <p,w> at pw), then z = M r.  Either leaves the n_rz partials of <r,z> and of the norm at rz / nn
  // (all-reduced into ctx->red with a communicator).
  virtual int apply(int it, const double* pw, int npw) = 0;
  virtual void end() {} // behind CgSolve::finish
};

struct ChebPc : CgPc
{
  using CgPc::CgPc;
  ChebPlan C;
  int setup() override
  {
    const int rc = chebyshev_setup(ctx, o, C);
    bound = C.hi;
    if (C.fused && C.degree > 1)
    {
      // the last term's partials sit behind the product's own (strides 1 and 2 of its partial array)
      rz = ctx->part_a.p + SPMV_PSTRIDE;
      nn = ctx->part_a.p + 2 * SPMV_PSTRIDE;
    }
    return rc;
  }
  int apply(int it, const double* pw, int npw) override
  {
    hipStream_t s = ctx->stream;
    const int* stop_flag = reinterpret_cast<const int*>(ctx->state.p);
    if (it < 0)
      cheb_first(ctx, ctx, C, ctx->r.p, nullptr, ctx->z.p);
    else
      hipLaunchKernelGGL(k_cheb_xr, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->alpha_hist.p, it, pw, npw, ctx->w.p,
                         ctx->dinv.p, C.theta, ctx->r.p, C.g, C.d, ctx->z.p, n);
    if (int rc = cheb_terms(ctx, ctx, C, ctx->r.p, ctx->z.p, o->norm, pa, pb, &n_rz))
      return rc;
    if (C.degree == 1)
      hipLaunchKernelGGL(k_dots_rz, dim3(g), dim3(VB), 0, s, stop_flag, ctx->r.p, ctx->z.p, n, o->norm, pa, pb);
    return ctx->comm ? comm_reduce_allreduce(ctx, stop_flag, rz, nn, nullptr, n_rz, 2, ctx->red.p) : ZZZ_OK;
  }
};

// "V-cycle, then k_dots_rz" in the polynomial's place; the cycle's own kernels return at once on the device's stop flag
struct MgPc : CgPc
{
  using CgPc::CgPc;
  int setup() override
  {
    prof_stride = 1; // (every product timed: about ten iterations of a few milliseconds each)
    poll_each = true;
    if (int rc = mg_setup(ctx, o)) // runs the levels' spectrum estimates through this context's CG vectors
      return rc;
    bound = mg_level0_bound(ctx);
    mg_profile_begin(ctx);
    return ZZZ_OK;
  }
  int apply(int it, const double* pw, int npw) override
  {
    hipStream_t s = ctx->stream;
    if (it >= 0)
      hipLaunchKernelGGL(k_update_xr<false>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->alpha_hist.p, it, pw, npw,
                         ctx->w.p, ctx->dinv.p, ctx->r.p, ctx->z.p, n, o->norm, pa, pb, o->variant, DinvCodes());
    if (int rc = mg_vcycle(ctx, ctx->r.p, ctx->z.p, o->profile != 0))
      return rc;
    const int* stop_flag = reinterpret_cast<const int*>(ctx->state.p);
    hipLaunchKernelGGL(k_dots_rz, dim3(g), dim3(VB), 0, s, stop_flag, ctx->r.p, ctx->z.p, n, o->norm, pa, pb);
    // (ZZZ_PC_MG on several ranks: the scalars of the owned entries, summed over the ranks as ChebPc's are)
    return ctx->comm ? comm_reduce_allreduce(ctx, stop_flag, rz, nn, nullptr, n_rz, 2, ctx->red.p) : ZZZ_OK;
  }
  // the cycle of the start-up and one per iteration that ran.  Behind a finish that failed (a HIP error) last_iters is the
  // solve's before and the mean says nothing; the call still runs, to hand the cycle's events back for the next solve.
  void end() override { mg_profile_end(ctx, o->profile ? ctx->last_iters + 1 : 0); }
};

static int cg_solve_pc(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm)
{
  ChebPc cheb(ctx, o);
  MgPc mg(ctx, o);
  CgPc& M = o->pc == ZZZ_PC_CHEBYSHEV_JACOBI ? static_cast<CgPc&>(cheb) : mg;
  const int64_t n = M.n;
  const int max_it = o->max_it, g = M.g;
  CgParams P{o->variant, ZZZ_PC_JACOBI, o->norm, o->rtol, o->atol, o->dtol > 0.0 ? o->dtol : 1.0e4};
  const bool multi = ctx->comm != nullptr;
  hipStream_t s = ctx->stream;
  if (int rc = M.setup())
    return rc;
  CgSolve S;
  if (int rc = S.begin(ctx, o, M.prof_stride))
    return rc;
  ZZZ_HIP(ctx, ctx->alpha_hist.reserve((size_t)max_it + 2));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->p.p, 0, sizeof(double) * ctx->p.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->u.p, 0, sizeof(double) * ctx->u.n, s)); // KSP zero initial guess
  hipLaunchKernelGGL(k_extract_dinv, dim3(g), dim3(VB), 0, s, ctx->rowptr.p, ctx->cols.p, ctx->vals.p, ctx->dinv.p, n, 1);
  // r = b
  hipLaunchKernelGGL(k_init_residual, dim3(g), dim3(VB), 0, s, ctx->b.p, (const double*)nullptr, ctx->dinv.p, ctx->r.p, ctx->z.p, n,
                     P.norm, M.pa, M.pb);
  if (int rc = M.apply(-1, nullptr, 0))
    return rc;
  const double *rz_src = M.rz, *nn_src = M.nn, *pw_src = ctx->part_a.p;
  int n_rz = M.n_rz;
  if (multi)
  {
    rz_src = ctx->red.p;
    nn_src = ctx->red.p + 1;
    pw_src = ctx->red.p + 2;
    n_rz = 1;
  }
  int it = 0;
  for (; it < max_it && !S.stop; ++it)
  {
    hipLaunchKernelGGL(k_update_p<false>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->dp_hist.p, ctx->alpha_hist.p,
                       it, P, rz_src, nn_src, n_rz, ctx->z.p, ctx->p.p, ctx->u.p, n, 1);
    const int slot = it % 2; // (poll_each: two of the skeleton's polling events; it waits for the copy it has just asked for)
    if (M.poll_each)
    {
      ZZZ_HIP(ctx, hipMemcpyAsync(&ctx->h_state[slot], ctx->state.p, sizeof(CgState), hipMemcpyDeviceToHost, s));
      ZZZ_HIP(ctx, hipEventRecord(S.chk_ev[slot], s));
    }
    int np = 0;
    S.product_begin(it);
    if (int rc = S.product_end(launch_product(ctx, ctx->p.p, ctx->w.p, ctx->part_a.p, &np)))
      return rc;
    if (multi)
    {
      if (int rc = comm_reduce_allreduce(ctx, reinterpret_cast<const int*>(ctx->state.p), ctx->part_a.p, nullptr, nullptr, np, 1,
                                         ctx->red.p + 2))
        return rc;
      np = 1;
    }
    if (int rc = M.apply(it, pw_src, np))
      return rc;
    if (M.poll_each)
    {
      ZZZ_HIP(ctx, hipEventSynchronize(S.chk_ev[slot]));
      if (ctx->h_state[slot].converged)
        S.stop = true;
    }
    else if (int rc = S.poll(it + 1))
      return rc;
  }
  hipLaunchKernelGGL(k_update_p<false>, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->dp_hist.p, ctx->alpha_hist.p, it,
                     P, rz_src, nn_src, n_rz, ctx->z.p, ctx->p.p, ctx->u.p, n, 0);
  ctx->last_pc_bound = M.bound;
  const int rc = S.finish(iters, rnorm);
  M.end();
  return rc;
}

// -ksp_cg_single_reduction: see k_sr_update.  Two kernels and one reduction point per iteration.
static int cg_solve_single_reduction(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm)
{
  const int64_t n = ctx->n_owned * ctx->bs;
  const int max_it = o->max_it;
  CgParams P{o->variant, o->pc, o->norm, o->rtol, o->atol, o->dtol > 0.0 ? o->dtol : 1.0e4};
  const bool multi = ctx->comm != nullptr;
  const int g = vgrid(n);
  hipStream_t s = ctx->stream;
  const int nn_is_rr = o->norm == ZZZ_NORM_UNPRECONDITIONED ? 1 : 0;
  // Chebyshev-Jacobi in this form: ONE reduction point per k products (the classical form has two) and k + 1 launches
  const bool cheb = o->pc == ZZZ_PC_CHEBYSHEV_JACOBI;
  ChebPlan C;
  if (cheb)
    if (int rc = chebyshev_setup(ctx, o, C))
      return rc;
  const bool ntv = loop_exceeds_cache(ctx, 8);

  CgSolve S;
  if (int rc = S.begin(ctx, o))
    return rc;
  ZZZ_HIP(ctx, ctx->dpi_hist.reserve((size_t)max_it + 2));
  ZZZ_HIP(ctx, ctx->sr_s.alloc((size_t)ctx->nloc()));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->p.p, 0, sizeof(double) * ctx->p.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->w.p, 0, sizeof(double) * ctx->w.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->z.p, 0, sizeof(double) * ctx->z.n, s)); // ghost entries of z are exchanged
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->u.p, 0, sizeof(double) * ctx->u.n, s)); // KSP zero initial guess
  hipLaunchKernelGGL(k_extract_dinv, dim3(g), dim3(VB), 0, s, ctx->rowptr.p, ctx->cols.p, ctx->vals.p, ctx->dinv.p, n,
                     o->pc != ZZZ_PC_NONE ? 1 : 0);
  // Jacobi's inverse diagonal as 16-bit codes, z of the last iteration recomputed from r (k_sr_update<.., DZ>): under the
  // rule of the classical form (a loop too large for the Infinity Cache; ZZZ_CG_DINV_CODES: 0 never, 2 at any size)
  DinvCodes dzc{nullptr, nullptr, nullptr, 0, 0};
  if (!cheb && o->pc == ZZZ_PC_JACOBI && ctx->knob.cg_dinv_codes != 0 && (ctx->knob.cg_dinv_codes >= 2 || ntv))
    if (int rc = dinv_codes_build(ctx, n, dzc))
      return rc;
  ctx->last_solve_dinv_codes = dzc.codes ? dzc.ndict : 0;
  ctx->last_solve_dinv_bits = dzc.codes ? dzc.bits : 0;
  auto kern_sr_update = cheb ? (ntv ? k_sr_update<true, true> : k_sr_update<false, true>)
                             : dz_dispatch(ntv, dz_form(dzc), [](auto NT, auto DZ) {
                                 return k_sr_update<decltype(NT)::value, false, decltype(DZ)::value>;
                               });
  // r = b, z = D^-1 r (the partials of this kernel are not used: the SpMV below leaves all three)
  hipLaunchKernelGGL(k_init_residual, dim3(g), dim3(VB), 0, s, ctx->b.p, (const double*)nullptr, ctx->dinv.p, ctx->r.p,
                     ctx->z.p, n, P.norm, ctx->part_b.p, ctx->part_b.p + VGRID_MAX);
  // ... or z = p_k(D^-1 A) D^-1 r: first term, then the others (none of them sums anything: the product s = A z does)
  auto polynomial = [&](bool first) -> int {
    if (!cheb)
      return ZZZ_OK;
    if (first)
      cheb_first(ctx, ctx, C, ctx->r.p, nullptr, ctx->z.p);
    return cheb_terms(ctx, ctx, C, ctx->r.p, ctx->z.p);
  };
  if (int rc = polynomial(true))
    return rc;

  double* parts = ctx->part_a.p; // <z,s> | <r,z> | norm, SPMV_PSTRIDE apart
  const double *zs_src = parts, *rz_src = parts + SPMV_PSTRIDE, *nn_src = parts + 2 * SPMV_PSTRIDE;
  if (multi)
  {
    rz_src = ctx->red.p;
    nn_src = ctx->red.p + 1;
    zs_src = ctx->red.p + 2;
  }
  int np = 0;
  // s = A z with the three partial dot products; then (multi) one all-reduce of three doubles
  auto apply = [&]() -> int {
    if (int rc = launch_product(ctx, ctx->z.p, ctx->sr_s.p, parts, &np, ctx->r.p, nn_is_rr))
      return rc;
    if (multi)
    {
      if (int rc = comm_reduce_allreduce(ctx, reinterpret_cast<const int*>(ctx->state.p), parts + SPMV_PSTRIDE,
                                         parts + 2 * SPMV_PSTRIDE, parts, np, 3, ctx->red.p))
        return rc;
      np = 1;
    }
    return ZZZ_OK;
  };

  if (int rc = apply())
    return rc;
  int it = 0;
  for (; it < max_it && !S.stop; ++it)
  {
    hipLaunchKernelGGL(kern_sr_update, dim3(g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->dpi_hist.p, ctx->dp_hist.p,
                       it, P, rz_src, nn_src, zs_src, np, ctx->dinv.p, ctx->sr_s.p, ctx->z.p, ctx->p.p, ctx->w.p, ctx->u.p,
                       ctx->r.p, n, 0, C.theta, C.g, C.d, dzc);
    if (int rc = polynomial(false))
      return rc;
    S.product_begin(it);
    if (int rc = S.product_end(apply()))
      return rc;
    if (int rc = S.poll(it + 1))
      return rc;
  }
  // convergence test of the last completed iteration: scalars only
  hipLaunchKernelGGL(kern_sr_update, dim3(1), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->dpi_hist.p, ctx->dp_hist.p, it,
                     P, rz_src, nn_src, zs_src, np, ctx->dinv.p, ctx->sr_s.p, ctx->z.p, ctx->p.p, ctx->w.p, ctx->u.p, ctx->r.p,
                     n, 1, C.theta, C.g, C.d, dzc);
  if (cheb)
    ctx->last_pc_bound = C.hi;
  return S.finish(iters, rnorm);
}
ZZZ_PRELOAD_TU(cg)
} // namespace zzz
