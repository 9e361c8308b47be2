// CSR SpMV for gfx950: y = A x, fp64 values / int32 columns (K6 of SURVEY.md 2c).
//
// Replaces PETSc MatMult inside KSPSolve (src/poisson_problem.cpp:177) and the `action` of
// linalg::cg (src/cg.h:62).  HBM-bound: 12 B per nonzero streamed once, x gathered through L2.
//
// Layout of the work: the nonzero stream is cut into row-aligned tiles of <= SPMV_TILE_NNZ entries and
// <= BLOCK rows.  A workgroup streams one tile's values and columns with 16-B / 8-B per-lane
// contiguous loads (every 128-B line of the matrix is fetched exactly once, fully coalesced),
// multiplies by the gathered x and parks the products in LDS; then one thread per row adds its
// products in column order -- the same order as a scalar CPU loop, so y is reproducible bit for bit.
// Workgroups are persistent (grid ~ 8 per CU) and walk the tiles XCD-aware: the workgroups that
// land on one XCD (blockIdx % 8, round-robin dispatch) sweep one contiguous eighth of the rows, so
// the x window they share stays in that XCD's 4 MiB L2 instead of being fetched by all eight.
#include <cstring>

#include <vector>

#include "zzz_device.h"
#include "zzz_internal.h"

namespace zzz
{
constexpr int SPMV_BLOCK = 256;

// One tile descriptor = {first row, end row, first nonzero, end nonzero}: one 16-B load per tile.
template <bool DOT, bool NT>
__global__ __launch_bounds__(SPMV_BLOCK, 8) void spmv_tile_kernel(const rp_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ cols,
                                                               const double* __restrict__ vals,
                                                               const double* __restrict__ x, double* __restrict__ y,
                                                               const int4* __restrict__ tiles, int64_t ntiles,
                                                               int nnz_even, double* __restrict__ partials,
                                                               const int* __restrict__ stop_flag,
                                                               const int32_t* __restrict__ tile_list,
                                                               const double* __restrict__ rvec, int pstride,
                                                               int nn_is_rr, const uint16_t* __restrict__ cols16,
                                                               const int32_t* __restrict__ tile_base, int offb,
                                                               int col_max, int lpr_shift)
{
  // lpr_shift > 0 (long rows: high order, vector-valued): 2^lpr_shift lanes share a row; lane j adds the
  // j-th contiguous chunk of ceil(len / lanes) products in column order and the chunk sums are combined by a
  // butterfly ((c0+c1)+(c2+c3))+...: a fixed order, restated by the oracle's zo_spmv_chunked.
  // cols16 != nullptr: 16-bit column codes (zzz_pattern.hip, k_tile_encode_cols): column = band base
  // of the tile [code >> offb] + (code & mask); the 2^(16-offb) band bases of a tile sit one per lane
  // in a register and are looked up with ds_bpermute.  Tiles whose columns do not fit (descriptor
  // .y < 0, holding ~r1) read the int32 columns.  Same columns, same arithmetic: results identical.
  // rvec != nullptr (single-reduction CG, x = z): besides <x,y> also leave the partials of <r,x> at
  // partials[pstride + b] and of the test norm (<x,x>, or <r,r> when nn_is_rr) at partials[2 pstride + b]
  // tile_list != nullptr: this launch covers only the listed tiles (interior or boundary subset of a
  // partitioned matrix); ntiles is then the length of the list
  if (stop_flag && *stop_flag) // CG already converged: the host is a few iterations ahead
    return;
  constexpr int TILE = SPMV_TILE_NNZ;
  __shared__ __attribute__((aligned(16))) double prod[TILE + 16];
  __shared__ double red[SPMV_BLOCK / 64];
  constexpr int NPASS = TILE / (2 * SPMV_BLOCK);
  RowSums S;
  dbl2 v[NPASS];
  int2v c[NPASS];
  int4 td = make_int4(0, 0, 0, 0);
  int bands = 0;
  const int nbands = 1 << (16 - offb);
  int64_t t = xcd_stride_item(ntiles, 0);
  // every matrix load is unconditional (indices clamped into the padded arrays), so all 2*NPASS
  // loads of a tile are in flight together, ahead of the 2*NPASS gathers that depend on them
  auto issue = [&](const int4 d, const int64_t tt) {
    const int s_al = d.z & ~1;
#pragma unroll
    for (int j = 0; j < NPASS; ++j)
    {
      const int kc = min(s_al + 2 * (int)threadIdx.x + j * 2 * SPMV_BLOCK, nnz_even);
      v[j] = vload<NT>(reinterpret_cast<const dbl2*>(vals + kc));
      if (cols16 && d.y >= 0) // packed columns: 4 B per pair instead of 8
        c[j].x = (int)vload<NT>(reinterpret_cast<const unsigned*>(cols16 + kc));
      else
        c[j] = vload<NT>(reinterpret_cast<const int2v*>(cols + kc));
    }
    if (cols16 && d.y >= 0)
      bands = tile_base[tt * nbands + (threadIdx.x & (nbands - 1))];
  };
  if (t >= 0)
  {
    const int64_t ti = tile_list ? tile_list[t] : t;
    td = tiles[ti];
    issue(td, ti);
  }
  for (int i = 0; t >= 0; ++i)
  {
    const int r0 = td.x, r1 = td.y < 0 ? ~td.y : td.y, s = td.z, e = td.w;
    const int s_al = s & ~1;
    double xa[NPASS], xb[NPASS];
    if (cols16 && td.y >= 0)
    {
      const unsigned mask = (1u << offb) - 1u;
#pragma unroll
      for (int j = 0; j < NPASS; ++j)
      {
        const unsigned u = (unsigned)c[j].x, lo = u & 0xffffu, hi = u >> 16;
        // window entries outside [s, e) carry another tile's codes: clamp, they are masked below
        c[j].x = min(__builtin_amdgcn_ds_bpermute((int)((lo >> offb) << 2), bands) + (int)(lo & mask), col_max);
        c[j].y = min(__builtin_amdgcn_ds_bpermute((int)((hi >> offb) << 2), bands) + (int)(hi & mask), col_max);
      }
    }
#pragma unroll
    for (int j = 0; j < NPASS; ++j)
    {
      xa[j] = x[c[j].x];
      xb[j] = x[c[j].y];
    }
    // this thread's row bounds (used after the barrier): issue the loads now
    const int r = r0 + (int)threadIdx.x;
    const int rc = min(r, r1 - 1);
    const int ra = (int)rowptr[rc] - s_al, rb = (int)rowptr[rc + 1] - s_al; // < 2^31 nonzeros on this path
    const double xr = DOT ? x[rc] : 0.0;
    const double rv = (DOT && rvec) ? rvec[rc] : 0.0;
#pragma unroll
    for (int j = 0; j < NPASS; ++j)
    {
      const int kk = s_al + 2 * (int)threadIdx.x + j * 2 * SPMV_BLOCK;
      if (kk < e)
      {
        dbl2 pr;
        pr.x = (kk >= s) ? v[j].x * xa[j] : 0.0;
        pr.y = (kk + 1 < e) ? v[j].y * xb[j] : 0.0;
        *reinterpret_cast<dbl2*>(prod + (kk - s_al)) = pr;
      }
    }
    const int64_t tn = xcd_stride_item(ntiles, i + 1);
    __syncthreads();
    if (lpr_shift == 0)
    {
      for (int rr = r; rr < r1; rr += SPMV_BLOCK) // one row per thread unless the rows are very short
      {
        const int ra_ = (rr == r) ? ra : (int)rowptr[rr] - s_al, rb_ = (rr == r) ? rb : (int)rowptr[rr + 1] - s_al;
        const double xr_ = (rr == r) ? xr : (DOT ? x[rr] : 0.0);
        // products are added in column order (the serial CPU order); 8 LDS reads in flight at a time
        double sum = 0.0;
        constexpr int QB = 8;
        for (int k = ra_; k < rb_; k += QB)
        {
          double q[QB];
  #pragma unroll
          for (int u = 0; u < QB; ++u)
            q[u] = prod[k + u]; // may run past the row: within the padded LDS array, masked below
  #pragma unroll
          for (int u = 0; u < QB; ++u)
            if (k + u < rb_)
              sum += q[u];
        }
        y[rr] = sum;
        if (DOT)
          row_sums(S, rvec != nullptr, nn_is_rr, sum, xr_, [&] { return (rr == r) ? rv : rvec[rr]; });
      }
    }
    else
    {
      const int lanes = 1 << lpr_shift, sub = (int)threadIdx.x & (lanes - 1);
      for (int rr = r0 + ((int)threadIdx.x >> lpr_shift); rr < r1; rr += SPMV_BLOCK >> lpr_shift)
      {
        const int ra_ = (int)rowptr[rr] - s_al, rb_ = (int)rowptr[rr + 1] - s_al;
        const int chunk = (rb_ - ra_ + lanes - 1) >> lpr_shift;
        const int ka = ra_ + sub * chunk, kb = min(ka + chunk, rb_);
        double sum = 0.0;
        for (int k = ka; k < kb; k += 4)
        {
          double q[4];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            q[u] = prod[min(k + u, TILE + 15)];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (k + u < kb)
              sum += q[u];
        }
        for (int o = 1; o < lanes; o <<= 1)
          sum += __shfl_xor(sum, o);
        if (sub == 0)
        {
          y[rr] = sum;
          if (DOT)
            row_sums(S, rvec != nullptr, nn_is_rr, sum, x[rr], [&] { return rvec[rr]; });
        }
      }
    }
    __syncthreads();
    t = tn;
    if (t >= 0)
    {
      const int64_t ti = tile_list ? tile_list[t] : t;
      td = tiles[ti];
      issue(td, ti);
    }
  }
  if (DOT)
    row_sums_store(S, rvec != nullptr, false, partials, pstride, red);
}

static int tile_grid(int64_t ntiles)
{
  // 8 workgroups of 256 threads per CU; always a multiple of 8 so that every XCD residue
  // (blockIdx % 8) that owns tiles in xcd_stride_item() has at least one workgroup
  int64_t g = 256 * 8;
  const int64_t need = (ntiles + 7) / 8 * 8;
  if (g > need)
    g = need;
  if (g < 8)
    g = 8;
  return (int)g;
}

// [mode][load].  The kernel takes rvec at run time, so the single-reduction form is the DOT instantiation, and it has no
// Chebyshev epilogue: those products need the operator stream.
using TileKernel = decltype(&spmv_tile_kernel<false, false>);
static const TileKernel tile_kernels[PM_PLAIN + 1][2] = {{spmv_tile_kernel<true, true>, spmv_tile_kernel<true, false>},
                                                         {spmv_tile_kernel<true, true>, spmv_tile_kernel<true, false>},
                                                         {spmv_tile_kernel<false, true>, spmv_tile_kernel<false, false>}};

// bit 0 of the variant: non-temporal matrix loads.  Unless a variant was forced, the load
// policy follows the matrix size: a matrix that fits the 256 MiB Infinity Cache is re-read from it
// every CG iteration, and non-temporal loads would throw that away (measured, 1.25 M-dof P1 matrix,
// 221 MB: 44 us plain vs 55 us nt; 2.5 M dofs and up: nt 2-8 % faster).
static ProductLoad tile_load(const zzz_ctx* ctx)
{
  int var = ctx->spmv_variant;
  if (ctx->spmv_auto)
    var = (var & ~1) | (12.0 * (double)ctx->nnz > 300.0e6 ? 1 : 0);
  return (var & 1) ? LOAD_NT : LOAD_PLAIN;
}

static void launch_variant(zzz_ctx* ctx, int grid, const ProductCall& c)
{
  const int4* tiles = reinterpret_cast<const int4*>(ctx->tile_row.p);
  const int64_t nt = c.list ? c.nlist : ctx->ntiles;
  const int nnz_even = (int)((ctx->nnz + 1) & ~(int64_t)1); // last valid clamped index (arrays are padded by 8)
  // bit 4 of the variant: ignore the packed columns (A/B and parity of the two index streams)
  const uint16_t* c16 = (ctx->pattern.have_cols16 && !(ctx->spmv_variant & 16)) ? ctx->cols16.p : nullptr;
  const int col_max = (int)ctx->nloc() - 1; // nloc() counts scalar entries (a clamp bs times too far read past the end of x)
  hipLaunchKernelGGL(tile_kernels[c.mode][c.load], dim3(grid), dim3(SPMV_BLOCK), 0, ctx->stream, ctx->rowptr.p, ctx->cols.p,
                     ctx->vals.p, c.x, c.y, tiles, nt, nnz_even, c.partials, c.stop, c.list, c.rvec, SPMV_PSTRIDE, c.nn_is_rr, c16,
                     ctx->tile_base.p, ctx->cols16_offb, col_max, ctx->spmv_lpr_shift);
}

// what a product on the tile kernel needs, whichever driver launches it
static int tile_prepare(zzz_ctx* ctx, ProductCall& c)
{
  if (c.epi)
    return fail(ctx, ZZZ_ERR_ARG, "a product with a Chebyshev term needs the operator stream (zzz_sellp.hip)");
  if (!ctx->tiles_ok)
    return fail(ctx, ZZZ_ERR_LIMIT, "%lld nonzeros: the product of a matrix of 2^31 nonzeros or more needs the operator stream "
                "(zzz_sellp.hip), which this matrix / these settings do not use", (long long)ctx->nnz);
  c.load = tile_load(ctx);
  return ensure_cols16(ctx);
}

int launch_spmv(zzz_ctx* ctx, const double* x, double* y, double* partials, int* npartials, const double* rvec, int nn_is_rr,
                const ChebEpi* epi)
{
  ProductCall c = product_call(ctx, x, y, partials, rvec, nn_is_rr, epi);
  if (sellp_active(ctx))
    return launch_sellp(ctx, c, npartials);
  if (int rc = tile_prepare(ctx, c))
    return rc;
  const int grid = tile_grid(ctx->ntiles);
  if (partials && (size_t)grid > ctx->part_a.n)
    return fail(ctx, ZZZ_ERR_ARG, "partials buffer too small");
  launch_variant(ctx, grid, c);
  if (partials && npartials)
    *npartials = grid;
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

// Partitioned matrix: y = A x with the forward halo of x overlapped with the interior items (tiles, groups of slices).
//   comm stream : (waits for x) pack + send/recv of the ghost entries        -- issued FIRST so that
//   main stream : product over the items that reference no ghost column         its kernels get CUs
//   main stream : (waits for the halo) product over the boundary items
// Partials of <x,y>: interior workgroups first, then the boundary ones.
int launch_overlapped(zzz_ctx* ctx, double* x, ProductCall c, const ProductPart& in, const ProductPart& bd, ProductLauncher launch,
                      int* npartials)
{
  int rc = comm_halo_begin(ctx, x);
  if (rc)
    return rc;
  c.list = in.list;
  c.nlist = in.n;
  if (in.n)
    launch(ctx, in.grid, c);
  rc = comm_halo_end(ctx);
  if (rc)
    return rc;
  c.list = bd.list;
  c.nlist = bd.n;
  if (c.partials)
    c.partials += in.grid;
  if (bd.n)
    launch(ctx, bd.grid, c);
  if (npartials)
    *npartials = in.grid + bd.grid;
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

static int launch_spmv_overlapped(zzz_ctx* ctx, double* x, double* y, double* partials, int* npartials, const double* rvec,
                                  int nn_is_rr, const ChebEpi* epi)
{
  ProductCall c = product_call(ctx, x, y, partials, rvec, nn_is_rr, epi);
  if (sellp_active(ctx) && ctx->pattern.have_group_split)
    return launch_sellp_overlapped(ctx, x, c, npartials);
  if (int rc = tile_prepare(ctx, c))
    return rc;
  const int64_t n_in = ctx->n_tiles_interior, n_bd = ctx->n_tiles_boundary;
  // The interior launch leaves one workgroup slot per CU free (7 of 8): at full occupancy the persistent
  // SpMV workgroups hold every wave slot until the launch ends and RCCL's send/recv kernel, although
  // enqueued first on a high-priority stream, could not start beside them -- no overlap at all.
  int g_in = n_in ? tile_grid(n_in) : 0;
  if (g_in > 256 * 7 && ctx->nneigh > 0)
    g_in = 256 * 7;
  const int g_bd = n_bd ? tile_grid(n_bd) : 0;
  if (partials && (size_t)(g_in + g_bd) > ctx->part_a.n)
    return fail(ctx, ZZZ_ERR_ARG, "partials buffer too small");
  return launch_overlapped(ctx, x, c, {n_in, ctx->tiles_interior.p, g_in}, {n_bd, ctx->tiles_boundary.p, g_bd}, launch_variant,
                           npartials);
}

int launch_product(zzz_ctx* ctx, double* x, double* y, double* partials, int* npartials, const double* rvec, int nn_is_rr,
                   const ChebEpi* epi)
{
  if (ctx->comm)
  {
    if (ctx->knob.overlap && ctx->pattern.have_tile_split)
      return launch_spmv_overlapped(ctx, x, y, partials, npartials, rvec, nn_is_rr, epi);
    if (int rc = comm_halo_forward(ctx, x))
      return rc;
  }
  return launch_spmv(ctx, x, y, partials, npartials, rvec, nn_is_rr, epi);
}
ZZZ_PRELOAD_TU(spmv)
} // namespace zzz
