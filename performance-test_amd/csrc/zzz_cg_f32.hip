// linalg::cg of src/cg.h:38-86 with U = float -- what the reference's cgpoisson runs when PETSc is built in single precision
// (`using T = PetscScalar`, src/cgpoisson_problem.cpp:28) -- on float device vectors x, r, p, y and the float action of
// zzz_matfree.hip.  A loop of its own (zzz_cg.hip's kernels gain no template axis), on one rank.
//
// One iteration k = 1, 2, ... is three launches:
//   action          y = A p with the partials of <p, y>                                            (src/cg.h:62)
//   k32_update_xr   alpha = rnorm / <p, y>;  x += alpha p;  r -= alpha y;  partials of <r, r>        (:65-71)
//   k32_update_p    rnorm_new, beta = rnorm_new / rnorm, the test rnorm_new / rnorm0 < rtol^2, the residual history and the
//                   stop flag;  p = beta p + r                                                     (:74-82)
// k32_init forms x = float(u) (the initial guess, :39), then r = b - y, p = r and the partials of <r, r> (:43-53).
//
// Scalars.  alpha and beta are floats, as `const U alpha` and `const U beta` are (:65,75); rnorm is a float as well
// (la::squared_norm returns U).  The sums behind them are ACCUMULATED IN DOUBLE and rounded once, where the reference
// accumulates in U: more accurate, and with the fixed trees below deterministic.  They live in device memory; every kernel
// returns at once when the stop flag is set, and the host looks at the state every 8 iterations, three batches behind the
// queue, exactly as cg_solve does.
#include "zzz_cg.h"
#include "zzz_device.h"
#include "zzz_internal.h"

#include <cmath>

namespace zzz
{
namespace
{
// one workgroup-wide sum of parts[0..np) in a fixed order; the result in every thread
__device__ inline double sum_parts_bcast(const double* __restrict__ parts, int np)
{
  __shared__ double sh[VB / 64];
  __shared__ double bc;
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += VB)
    s += parts[i];
  const double t = block_reduce_sum(s, sh);
  if (threadIdx.x == 0)
    bc = t;
  __syncthreads();
  return bc;
}

// phase 0: x = float(u) (before the first action); phase 1: r = float(b) - y, p = r, partials of <r, r>
__global__ __launch_bounds__(VB) void k32_init(int phase, const double* __restrict__ b, const double* __restrict__ u,
                                               const float* __restrict__ y, float* __restrict__ x, float* __restrict__ r,
                                               float* __restrict__ p, int64_t n, double* __restrict__ parts)
{
  __shared__ double sh[VB / 64];
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    if (phase == 0)
      x[i] = (float)u[i];
    else
    {
      const float ri = (float)b[i] - y[i]; // axpy(r, U(-1), y, b), src/cg.h:47
      r[i] = ri;
      p[i] = ri;
      acc += (double)ri * (double)ri;
    }
  }
  if (phase != 0)
  {
    const double t = block_reduce_sum(acc, sh);
    if (threadIdx.x == 0)
      parts[blockIdx.x] = t;
  }
}

// iteration it (1-based): beta_hist[it - 1] holds rnorm as update_p left it
__global__ __launch_bounds__(VB) void k32_update_xr(const CgState* __restrict__ st, const double* __restrict__ beta_hist, int it,
                                                    const double* __restrict__ pw_parts, int npw, const float* __restrict__ p,
                                                    const float* __restrict__ y, float* __restrict__ x, float* __restrict__ r,
                                                    int64_t n, double* __restrict__ parts)
{
  if (st->converged) // (set by an earlier launch)
    return;
  __shared__ double sh[VB / 64];
  const float rnorm = (float)beta_hist[it - 1];
  const float pw = (float)sum_parts_bcast(pw_parts, npw); // la::inner_product(p, y), src/cg.h:65
  const float alpha = rnorm / pw;
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    x[i] = alpha * p[i] + x[i];          // axpy(x, alpha, p, x), :68
    const float ri = -alpha * y[i] + r[i]; // axpy(r, -alpha, y, r), :71
    r[i] = ri;
    acc += (double)ri * (double)ri;
  }
  const double t = block_reduce_sum(acc, sh);
  if (threadIdx.x == 0)
    parts[blockIdx.x] = t;
}

// it = 0: records rnorm0 (no test, p = r already); it >= 1: the tail of iteration it
__global__ __launch_bounds__(VB) void k32_update_p(CgState* __restrict__ st, double* __restrict__ beta_hist, double* __restrict__ dp_hist,
                                                   int it, double rtol2, const double* __restrict__ rr_parts, int nrr,
                                                   const float* __restrict__ r, float* __restrict__ p, int64_t n)
{
  // stopped by an EARLIER launch (workgroup 0 of this very launch may be setting the words while others start: conv_it1 tells
  // the two apart, as in zzz_cg.hip)
  const int c = __atomic_load_n(&st->conv_it1, __ATOMIC_RELAXED);
  const double dp0_st = st->dp0;
  const double prev = it > 0 ? beta_hist[it - 1] : 0.0;
  if (c != 0 && c - 1 < it)
    return;
  const float rnorm_new = (float)sum_parts_bcast(rr_parts, nrr); // la::squared_norm(r), :53,74
  const float rnorm0 = it == 0 ? rnorm_new : (float)dp0_st;
  const float beta = it == 0 ? 0.0f : rnorm_new / (float)prev; // const U beta, :75
  const bool conv = it > 0 && (double)rnorm_new / (double)rnorm0 < rtol2; // :78 (strict; no test before the first iteration)
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    beta_hist[it] = (double)rnorm_new;
    dp_hist[it] = (double)rnorm_new;
    st->dp = (double)rnorm_new;
    if (it == 0)
    {
      st->dp0 = (double)rnorm_new;
      st->ttol = rtol2;
    }
    if (conv)
    {
      st->iters = it;
      st->converged = 1; // the other workgroups reach the same verdict from the same partials
      __atomic_store_n(&st->conv_it1, it + 1, __ATOMIC_RELAXED);
    }
  }
  if (conv || it == 0)
    return; // `break` comes before the direction update, :78-82
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    p[i] = beta * p[i] + r[i]; // axpy(p, beta, p, r), :82
}

__global__ __launch_bounds__(VB) void k32_store_u(const float* __restrict__ x, double* __restrict__ u, int64_t n)
{
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
    u[i] = (double)x[i];
}
} // namespace

int cg_solve_f32(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm)
{
  cg_report_reset(ctx);
  const int64_t n = ctx->n_owned; // (block size 1, one rank: no ghosts)
  const size_t nl = (size_t)ctx->nloc();
  const int max_it = o->max_it;
  const int g = vgrid(n);
  hipStream_t s = ctx->stream;

  // a mesh the float action refuses is refused before the solve touches anything
  if (int rc = mf_f32_prepare(ctx))
    return rc;
  // grow-only: nothing is freed on the solve path
  ZZZ_HIP(ctx, ctx->f32_x.reserve(nl));
  ZZZ_HIP(ctx, ctx->f32_r.reserve(nl));
  ZZZ_HIP(ctx, ctx->f32_p.reserve(nl));
  ZZZ_HIP(ctx, ctx->f32_y.reserve(nl));
  CgSolve S;
  if (int rc = S.begin(ctx, o))
    return rc;
  CgState* const st = ctx->state.p;
  float *x = ctx->f32_x.p, *r = ctx->f32_r.p, *p = ctx->f32_p.p, *y = ctx->f32_y.p;
  double* rr_parts = ctx->part_b.p; // g <= VGRID_MAX entries
  double* pw_parts = ctx->part_a.p; // the action's: its workgroups, then its finish kernel's
  const double rtol2 = o->rtol * o->rtol;

  // r0 = b - A x0, p = r0 (src/cg.h:43-50)
  hipLaunchKernelGGL(k32_init, dim3(g), dim3(VB), 0, s, 0, ctx->b.p, ctx->u.p, (const float*)nullptr, x, r, p, n, rr_parts);
  if (int rc = mf_action_f32(ctx, x, y, nullptr, nullptr))
    return rc;
  hipLaunchKernelGGL(k32_init, dim3(g), dim3(VB), 0, s, 1, ctx->b.p, ctx->u.p, y, x, r, p, n, rr_parts);
  hipLaunchKernelGGL(k32_update_p, dim3(g), dim3(VB), 0, s, st, ctx->beta_hist.p, ctx->dp_hist.p, 0, rtol2, rr_parts, g, r, p, n);

  for (int it = 1; it <= max_it && !S.stop; ++it)
  {
    int np = 0;
    if (int rc = mf_action_f32(ctx, p, y, pw_parts, &np))
      return rc;
    hipLaunchKernelGGL(k32_update_xr, dim3(g), dim3(VB), 0, s, st, ctx->beta_hist.p, it, pw_parts, np, p, y, x, r, n, rr_parts);
    hipLaunchKernelGGL(k32_update_p, dim3(g), dim3(VB), 0, s, st, ctx->beta_hist.p, ctx->dp_hist.p, it, rtol2, rr_parts, g, r, p, n);
    if (int rc = S.poll(it))
      return rc;
  }
  // the solution into the context's u, as doubles: zzz_vec_download, zzz_vec_norm and the driver's --output see it there
  hipLaunchKernelGGL(k32_store_u, dim3(g), dim3(VB), 0, s, x, ctx->u.p, n);
  return S.finish(iters, rnorm);
}
ZZZ_PRELOAD_TU(cg_f32)
} // namespace zzz
