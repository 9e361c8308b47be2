// Pipelined conjugate gradients: PETSc's KSPPIPECG (-ksp_type pipecg; Ghysels & Vanroose, "Hiding global
// synchronization latency in the preconditioned Conjugate Gradient algorithm", Parallel Computing 40, 2014, Alg. 4),
// left-preconditioned with M = Jacobi's D (or I), zero initial guess, on the assembled operator.  ZZZ_CG_PIPE.
//
//   r = b;  u = M^-1 r;  w = A u
//   for i = 0, 1, ...
//     gamma = <r,u>;  delta = <w,u>;  dp = ||u|| | ||r|| | sqrt|gamma|      <- ONE reduction of three sums ...
//     m = M^-1 w;  n = A m                                                  <- ... that runs WHILE the product does
//     test dp (KSPConvergedDefault)
//     i == 0:  alpha = gamma / delta;  z = n;  p = u;  s = w
//     else:    beta = gamma / gamma_old;  alpha = gamma / (delta - beta gamma / alpha_old)
//              z = n + beta z;  p = u + beta p;  s = w + beta s             (q = m + beta q = D^-1 s: never formed)
//     x += alpha p;  r -= alpha s;  w -= alpha z                            (u -= alpha q = D^-1 r: recomputed)
//
// One iteration is TWO launches on the main stream: k_pipe_update (everything but the product, one pass over the
// vectors) and the product n = A m on whatever form the matrix took (launch_product; the partials
// the product leaves are not used).  k_pipe_update(i) takes the reduced (gamma, delta, norm^2) of iteration i, tests,
// forms alpha and beta, updates z, p, s, x, r, w, writes m = D^-1 w for the product to gather and leaves the block
// partials of gamma, delta and norm^2 of iteration i + 1.
//
// The preconditioned vectors are not stored: u = D^-1 r and q = D^-1 s hold by construction, so u is recomputed from r
// (before the update for p, after it for the sums) and q is not needed at all.  Per row and iteration the kernel reads
// n, z, s, p, x, r, w and writes z, s, p, x, r, w, m: 7 + 7 vectors = 112 B, + 8 B of D^-1 as doubles or 2 B as the
// 16-bit codes of dinv_codes_build (under the rule of the other forms), against 144 B with u and q stored.
//
// With a communicator attached the all-reduce of the three sums is enqueued by comm_reduce_begin -- on a stream of its
// own, behind an event recorded after k_pipe_update(i) -- so that it does not order before the halo exchange and the
// product of the same iteration; k_pipe_update(i + 1) waits for its event (comm_reduce_end).  A single rank sums the
// partials in the kernel's prologue as the other forms do: no second stream.
#include "zzz_cg.h"

#include <algorithm>
#include <cmath>

namespace zzz
{
// the first sums: u = D^-1 r, m = D^-1 w; partials of <r,u>, <w,u> and the test norm^2 (r = b and w = A u are there)
__global__ __launch_bounds__(VB) void k_pipe_start(const double* __restrict__ dinv, const double* __restrict__ r,
                                                   const double* __restrict__ w, double* __restrict__ m, int64_t n, int norm,
                                                   double* __restrict__ qa, double* __restrict__ qb, double* __restrict__ qc)
{
  __shared__ double sh[VB / 64];
  double sa = 0, sb = 0, sc = 0;
  for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < n; i += (int64_t)gridDim.x * VB)
  {
    const double di = dinv[i], ri = r[i], wi = w[i];
    const double ui = di * ri;
    m[i] = di * wi;
    sa += ri * ui;
    sb += wi * ui;
    sc += (norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : ui * ui;
  }
  const double ta = block_reduce_sum(sa, sh);
  const double tb = block_reduce_sum(sb, sh);
  const double tc = block_reduce_sum(sc, sh);
  if (threadIdx.x == 0)
  {
    qa[blockIdx.x] = ta;
    qb[blockIdx.x] = tb;
    qc[blockIdx.x] = tc;
  }
}

// `it` = number of completed iterations.  pa/pb/pc: partials (np each) or the single all-reduced values (np == 1) of
// gamma = <r,u>, delta = <w,u> and the test norm^2 of iteration `it`; qa/qb/qc: where this launch leaves the partials of
// iteration it + 1 (another set than pa/pb/pc: workgroups of one launch read the one while others already write the
// other).  nv = A m of this iteration.  scalars_only: the test of the last completed iteration (one workgroup).
// DZ: D^-1 as codes into a table in LDS (DinvCodes), 2 B per row instead of 8 (DZ = 1, 16-bit codes) or 1 B (DZ = 2, 8-bit
// codes); DZ = 0: doubles.
template <bool NT, int DZ>
__global__ __launch_bounds__(VB) void k_pipe_update(CgState* __restrict__ st, double* __restrict__ gamma_hist,
                                                    double* __restrict__ alpha_hist, double* __restrict__ dp_hist, int it,
                                                    CgParams P, const double* __restrict__ pa, const double* __restrict__ pb,
                                                    const double* __restrict__ pc, int np, const double* __restrict__ dinv,
                                                    const double* __restrict__ nv, double* __restrict__ z,
                                                    double* __restrict__ s, double* __restrict__ p, double* __restrict__ x,
                                                    double* __restrict__ r, double* __restrict__ w, double* __restrict__ m,
                                                    int64_t n, int scalars_only, double* __restrict__ qa,
                                                    double* __restrict__ qb, double* __restrict__ qc, DinvCodes dz)
{
  __shared__ double dtab[dz_table(DZ)];
  dz_stage<DZ>(dtab, dz);
  // first entries requested before the scalar prologue (see k_update_p of zzz_cg.hip): up to eight 16-B loads in flight
  // per thread while the workgroup walks the flag, the three sums and the convergence logic
  const int64_t n2 = n >> 1, stride = (int64_t)gridDim.x * VB;
  const int64_t i0 = blockIdx.x * (int64_t)VB + threadIdx.x;
  const dbl2* __restrict__ n2v = reinterpret_cast<const dbl2*>(nv);
  const dbl2* __restrict__ d2 = reinterpret_cast<const dbl2*>(dinv);
  dbl2 *__restrict__ z2 = reinterpret_cast<dbl2*>(z), *__restrict__ s2 = reinterpret_cast<dbl2*>(s),
                     *__restrict__ p2 = reinterpret_cast<dbl2*>(p), *__restrict__ x2 = reinterpret_cast<dbl2*>(x),
                     *__restrict__ r2 = reinterpret_cast<dbl2*>(r), *__restrict__ w2 = reinterpret_cast<dbl2*>(w),
                     *__restrict__ m2 = reinterpret_cast<dbl2*>(m);
  const int64_t c0 = (i0 < n2) ? i0 : 0;
  dbl2 ni0 = {0, 0}, zo0 = {0, 0}, so0 = {0, 0}, po0 = {0, 0}, xi0 = {0, 0}, ri0 = {0, 0}, wi0 = {0, 0}, di0 = {0, 0};
  uint32_t dc0 = 0;
  if (n2 > 0 && !scalars_only)
  {
    if (DZ)
      dc0 = dz_load2<DZ>(dz, c0);
    else
      di0 = vload<NT>(d2 + c0);
    ni0 = vload<NT>(n2v + c0);
    ri0 = vload<NT>(r2 + c0);
    wi0 = vload<NT>(w2 + c0);
    xi0 = vload<NT>(x2 + c0);
    zo0 = vload<NT>(z2 + c0); // zero before the first iteration (cg_solve_pipe clears z, s and p)
    so0 = vload<NT>(s2 + c0);
    po0 = vload<NT>(p2 + c0);
  }
  // ... and so are the scalar inputs: flag, tolerances, last iteration's coefficients, and (communicator attached:
  // np == 1) the three all-reduced sums themselves
  const int f0 = st->converged;
  const double ttol_st = st->ttol, dp0_st = st->dp0;
  const double go_h = it > 0 ? gamma_hist[it - 1] : 1.0, ao_h = it > 0 ? alpha_hist[it - 1] : 1.0;
  double gamma = pa[0], delta = pb[0], nn = pc[0];
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
    reduce_parts3_bcast(pa, pb, pc, np, gamma, delta, nn);
  }
  const double dp = (P.norm == ZZZ_NORM_NATURAL) ? sqrt(fabs(gamma)) : sqrt(nn);
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
  double beta = 0.0, alpha = gamma / delta;
  if (it > 0)
  {
    beta = gamma / go_h;
    alpha = gamma / (delta - beta * gamma / ao_h);
  }
  if (!conv && !scalars_only && !isfinite(alpha))
    conv = 2; // KSP_DIVERGED_NANORINF, as the other forms stop on a non-finite step length
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    gamma_hist[it] = gamma;
    alpha_hist[it] = alpha;
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
  __shared__ double sh[VB / 64];
  double sa = 0, sb = 0, sc = 0;
  for (int64_t i = i0; i < n2; i += stride)
  {
    // cache policy: only m (gathered by the product that follows) and n (its output) are worth keeping; the other
    // vectors are touched by this kernel alone, once per iteration
    dbl2 ni, zo, so, po, xi, ri, wi, di;
    uint32_t dc = dc0;
    if (i == i0)
    {
      ni = ni0, zo = zo0, so = so0, po = po0, xi = xi0, ri = ri0, wi = wi0, di = di0;
    }
    else
    {
      if (DZ)
        dc = dz_load2<DZ>(dz, i);
      else
        di = vload<NT>(d2 + i);
      ni = vload<NT>(n2v + i), ri = vload<NT>(r2 + i), wi = vload<NT>(w2 + i), xi = vload<NT>(x2 + i);
      if (it != 0)
        zo = vload<NT>(z2 + i), so = vload<NT>(s2 + i), po = vload<NT>(p2 + i);
    }
    if (DZ)
    {
      di.x = dtab[dz_lo<DZ>(dc)];
      di.y = dtab[dz_hi<DZ>(dc)];
    }
    dbl2 ui, zn = ni, sn = wi, pn, un, mn;
    ui.x = di.x * ri.x; // u = D^-1 r as the last launch formed it for its sums
    ui.y = di.y * ri.y;
    pn = ui;
    if (it != 0)
    {
      zn.x = beta * zo.x + ni.x;
      zn.y = beta * zo.y + ni.y;
      sn.x = beta * so.x + wi.x;
      sn.y = beta * so.y + wi.y;
      pn.x = beta * po.x + ui.x;
      pn.y = beta * po.y + ui.y;
    }
    xi.x = alpha * pn.x + xi.x;
    xi.y = alpha * pn.y + xi.y;
    ri.x = -alpha * sn.x + ri.x;
    ri.y = -alpha * sn.y + ri.y;
    wi.x = -alpha * zn.x + wi.x;
    wi.y = -alpha * zn.y + wi.y;
    un.x = di.x * ri.x;
    un.y = di.y * ri.y;
    mn.x = di.x * wi.x;
    mn.y = di.y * wi.y;
    vstore<NT>(zn, z2 + i);
    vstore<NT>(sn, s2 + i);
    vstore<NT>(pn, p2 + i);
    vstore<NT>(xi, x2 + i);
    vstore<NT>(ri, r2 + i);
    vstore<NT>(wi, w2 + i);
    m2[i] = mn;
    sa += ri.x * un.x;
    sa += ri.y * un.y;
    sb += wi.x * un.x;
    sb += wi.y * un.y;
    if (P.norm == ZZZ_NORM_UNPRECONDITIONED)
    {
      sc += ri.x * ri.x;
      sc += ri.y * ri.y;
    }
    else
    {
      sc += un.x * un.x;
      sc += un.y * un.y;
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
  {
    const int64_t i = n - 1;
    const double dv = DZ ? dtab[dz_load1<DZ>(dz, i)] : dinv[i];
    const double ui = dv * r[i];
    const double zn = (it == 0) ? nv[i] : beta * z[i] + nv[i];
    const double sn = (it == 0) ? w[i] : beta * s[i] + w[i];
    const double pn = (it == 0) ? ui : beta * p[i] + ui;
    z[i] = zn;
    s[i] = sn;
    p[i] = pn;
    x[i] = alpha * pn + x[i];
    const double ri = -alpha * sn + r[i];
    const double wi = -alpha * zn + w[i];
    r[i] = ri;
    w[i] = wi;
    const double un = dv * ri;
    m[i] = dv * wi;
    sa += ri * un;
    sb += wi * un;
    sc += (P.norm == ZZZ_NORM_UNPRECONDITIONED) ? ri * ri : un * un;
  }
  const double ta = block_reduce_sum(sa, sh);
  const double tb = block_reduce_sum(sb, sh);
  const double tc = block_reduce_sum(sc, sh);
  if (threadIdx.x == 0)
  {
    qa[blockIdx.x] = ta;
    qb[blockIdx.x] = tb;
    qc[blockIdx.x] = tc;
  }
}

int cg_solve_pipe(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm)
{
  const int64_t n = ctx->n_owned * ctx->bs;
  const int max_it = o->max_it;
  CgParams P{o->variant, o->pc, o->norm, o->rtol, o->atol, o->dtol > 0.0 ? o->dtol : 1.0e4};
  const bool multi = ctx->comm != nullptr;
  const int g = vgrid(n);
  hipStream_t s = ctx->stream;
  const bool ntv = loop_exceeds_cache(ctx, 10);

  CgSolve S;
  if (int rc = S.begin(ctx, o)) // (beta_hist: gamma)
    return rc;
  ZZZ_HIP(ctx, ctx->alpha_hist.reserve((size_t)max_it + 2));
  ZZZ_HIP(ctx, ctx->sr_s.alloc((size_t)ctx->nloc()));
  ZZZ_HIP(ctx, ctx->pipe_m.alloc((size_t)ctx->nloc()));
  ZZZ_HIP(ctx, ctx->pipe_n.alloc((size_t)ctx->nloc()));
  ZZZ_HIP(ctx, ctx->pipe_parts.reserve((size_t)(2 * 3 * VGRID_MAX)));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->z.p, 0, sizeof(double) * ctx->z.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->sr_s.p, 0, sizeof(double) * ctx->sr_s.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->p.p, 0, sizeof(double) * ctx->p.n, s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->pipe_m.p, 0, sizeof(double) * ctx->pipe_m.n, s)); // ghost entries of m are exchanged
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->u.p, 0, sizeof(double) * ctx->u.n, s));           // KSP zero initial guess
  cg_launch_extract_dinv(ctx, n, o->pc == ZZZ_PC_JACOBI ? 1 : 0);
  // Jacobi's inverse diagonal as 16-bit codes: under the rule of the other forms (a loop too large for the Infinity
  // Cache; ZZZ_CG_DINV_CODES: 0 never, 2 at any size)
  DinvCodes dzc{nullptr, nullptr, nullptr, 0, 0};
  if (o->pc == ZZZ_PC_JACOBI && ctx->knob.cg_dinv_codes != 0 && (ctx->knob.cg_dinv_codes >= 2 || ntv))
    if (int rc = dinv_codes_build(ctx, n, dzc))
      return rc;
  ctx->last_solve_dinv_codes = dzc.codes ? dzc.ndict : 0;
  ctx->last_solve_dinv_bits = dzc.codes ? dzc.bits : 0;
  auto kern = dz_dispatch(ntv, dz_form(dzc), [](auto NT, auto DZ) { return k_pipe_update<decltype(NT)::value, decltype(DZ)::value>; });

  double *x = ctx->u.p, *r = ctx->r.p, *w = ctx->w.p, *m = ctx->pipe_m.p, *nvec = ctx->pipe_n.p;
  // y = A v on the form the matrix took; the partials of <v,y> the product leaves in part_a are not used (asking for
  // them makes the launches behind a converged solve return at once, as in the other forms)
  auto apply = [&](double* v, double* y) -> int {
    int np = 0;
    return launch_product(ctx, v, y, ctx->part_a.p, &np);
  };
  // the two sets of partials, and where the kernel of iteration `it` finds its sums
  auto parts = [&](int it) { return ctx->pipe_parts.p + (size_t)(it & 1) * 3 * VGRID_MAX; };
  const int* stop_flag = reinterpret_cast<const int*>(ctx->state.p); // CgState::converged
  // (multi) the all-reduce of the sums of iteration `it`, begun behind the kernel that left their partials
  auto reduce_begin = [&](int it) -> int {
    if (!multi)
      return ZZZ_OK;
    double* q = parts(it);
    return comm_reduce_begin(ctx, stop_flag, q, q + VGRID_MAX, q + 2 * VGRID_MAX, g, 3, ctx->red.p);
  };
  auto update = [&](int it, int scalars_only) -> int {
    if (int rc = comm_reduce_end(ctx)) // the main stream meets the sums of iteration `it`
      return rc;
    const double* q = multi ? ctx->red.p : parts(it);
    const int qs = multi ? 1 : VGRID_MAX;
    double* qn = parts(it + 1);
    hipLaunchKernelGGL(kern, dim3(scalars_only ? 1 : g), dim3(VB), 0, s, ctx->state.p, ctx->beta_hist.p, ctx->alpha_hist.p,
                       ctx->dp_hist.p, it, P, q, q + qs, q + 2 * qs, multi ? 1 : g, ctx->dinv.p, nvec, ctx->z.p, ctx->sr_s.p,
                       ctx->p.p, x, r, w, m, n, scalars_only, qn, qn + VGRID_MAX, qn + 2 * VGRID_MAX, dzc);
    return ZZZ_OK;
  };

  // r = b, u = D^-1 r (into m's buffer: the product gathers it); w = A u; then m = D^-1 w and the first partials
  cg_launch_init_residual(ctx, m, n, P.norm, ctx->part_b.p, ctx->part_b.p + VGRID_MAX);
  if (int rc = apply(m, w))
    return rc;
  {
    double* q = parts(0);
    hipLaunchKernelGGL(k_pipe_start, dim3(g), dim3(VB), 0, s, ctx->dinv.p, r, w, m, n, P.norm, q, q + VGRID_MAX, q + 2 * VGRID_MAX);
  }
  if (int rc = reduce_begin(0))
    return rc;

  // n = A m of iteration 0, beside the first all-reduce
  if (int rc = apply(m, nvec))
    return rc;
  int it = 0;
  for (; it < max_it && !S.stop; ++it)
  {
    if (int rc = update(it, 0))
      return rc;
    if (int rc = reduce_begin(it + 1)) // ... beside the halo exchange and the product below
      return rc;
    S.product_begin(it);
    if (int rc = S.product_end(apply(m, nvec)))
      return rc;
    if (int rc = S.poll(it + 1))
      return rc;
  }
  // convergence test of the last completed iteration: scalars only
  if (int rc = update(it, 1))
    return rc;
  return S.finish(iters, rnorm);
}
ZZZ_PRELOAD_TU(cg_pipe)
} // namespace zzz
