// ZZZ_PC_PMG: the two transfer kernels between the Pk and the P1 dofs of one generated cube and their launches; what a
// thread does is in zzz_pmg.h.
#include "zzz_cg.h"
#include "zzz_pmg.h"

namespace zzz
{
using zzzcube::Layout;

template <int ORDER, int BS>
__global__ __launch_bounds__(VB) void k_pmg_prolong(const int* __restrict__ stop, Layout L, const uint8_t* __restrict__ bcf,
                                                    const uint8_t* __restrict__ bcc, const double* __restrict__ ec,
                                                    double* __restrict__ xf, int accumulate)
{
  if (stop && *stop)
    return;
  const int64_t n = L.PX * L.PY * (L.nz + 1) * BS;
  const int64_t u = blockIdx.x * (int64_t)VB + threadIdx.x;
  if (u < n)
    pmg_prolong_entry<ORDER, BS>(L, u, bcf, bcc, ec, xf, accumulate);
}
template <int ORDER, int BS>
__global__ __launch_bounds__(VB) void k_pmg_restrict(const int* __restrict__ stop, Layout L, const uint8_t* __restrict__ bcf,
                                                     const uint8_t* __restrict__ bcc, const double* __restrict__ rf,
                                                     const double* __restrict__ sub, double* __restrict__ rc)
{
  if (stop && *stop)
    return;
  const int64_t n = L.PX * L.PY * (L.nz + 1) * BS;
  const int64_t u = blockIdx.x * (int64_t)VB + threadIdx.x;
  if (u < n)
    pmg_restrict_entry<ORDER, BS>(L, u, bcf, bcc, rf, sub, rc);
}

// one thread per (lattice point, component): a thread stores up to 20 or gathers up to 65 entries, so nothing is strided; without
// the stride loop hipcc has no loop to hoist Layout's offsets out of, which kept 24 of them in spilled SGPRs at P3, block size 3
static unsigned pmg_grid(const Layout& L, int bs)
{
  const int64_t n = L.PX * L.PY * (L.nz + 1) * bs;
  return (unsigned)((n + VB - 1) / VB);
}

static bool pmg_shape(zzz_ctx* ctx, int order, int bs)
{
  if ((order == 2 || order == 3) && (bs == 1 || bs == 3))
    return true;
  fail(ctx, ZZZ_ERR_ARG, "-pc_type pmg: no transfer kernel for order %d, block size %d", order, bs);
  return false;
}

int pmg_prolong(zzz_ctx* ctx, const int* stop, int order, int bs, const int64_t n[3], const uint8_t* bcf, const uint8_t* bcc,
                const double* ec, double* xf, int accumulate)
{
  if (!pmg_shape(ctx, order, bs))
    return ZZZ_ERR_ARG;
  const Layout L(n[0], n[1], n[2], order);
  const dim3 g(pmg_grid(L, bs)), b(VB);
  hipStream_t s = ctx->stream;
  if (order == 2 && bs == 1)
    hipLaunchKernelGGL((k_pmg_prolong<2, 1>), g, b, 0, s, stop, L, bcf, bcc, ec, xf, accumulate);
  else if (order == 2)
    hipLaunchKernelGGL((k_pmg_prolong<2, 3>), g, b, 0, s, stop, L, bcf, bcc, ec, xf, accumulate);
  else if (bs == 1)
    hipLaunchKernelGGL((k_pmg_prolong<3, 1>), g, b, 0, s, stop, L, bcf, bcc, ec, xf, accumulate);
  else
    hipLaunchKernelGGL((k_pmg_prolong<3, 3>), g, b, 0, s, stop, L, bcf, bcc, ec, xf, accumulate);
  return ZZZ_OK;
}

int pmg_restrict(zzz_ctx* ctx, const int* stop, int order, int bs, const int64_t n[3], const uint8_t* bcf, const uint8_t* bcc,
                 const double* rf, const double* sub, double* rc)
{
  if (!pmg_shape(ctx, order, bs))
    return ZZZ_ERR_ARG;
  const Layout L(n[0], n[1], n[2], order);
  const dim3 g(pmg_grid(L, bs)), b(VB);
  hipStream_t s = ctx->stream;
  if (order == 2 && bs == 1)
    hipLaunchKernelGGL((k_pmg_restrict<2, 1>), g, b, 0, s, stop, L, bcf, bcc, rf, sub, rc);
  else if (order == 2)
    hipLaunchKernelGGL((k_pmg_restrict<2, 3>), g, b, 0, s, stop, L, bcf, bcc, rf, sub, rc);
  else if (bs == 1)
    hipLaunchKernelGGL((k_pmg_restrict<3, 1>), g, b, 0, s, stop, L, bcf, bcc, rf, sub, rc);
  else
    hipLaunchKernelGGL((k_pmg_restrict<3, 3>), g, b, 0, s, stop, L, bcf, bcc, rf, sub, rc);
  return ZZZ_OK;
}
ZZZ_PRELOAD_TU(pmg)
} // namespace zzz
