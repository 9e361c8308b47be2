// The CG operator stream, part 3 of 3: the PRODUCT on the stream the packer (zzz_sellp_pack.hip) and the dictionary builders
// (zzz_sellp_dict.hip) leave; streams of one-chunk slices on coded values have a kernel of their own (zzz_sellp_pipe.hip).
// The stream's format is described at the head of zzz_sellp_pack.hip.
#include <climits>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "zzz_sellp.h"

namespace zzz
{
// ---- the product --------------------------------------------------------------------------------------
// Values and columns of chunk c for this lane.  FULL: all eight slots (every chunk but the last of a slice);
// otherwise only the first w: unused value blocks are not loaded (an odd w loads its last entry with one 8-B load).
// Columns by the chunk's mode (meta[c][0]: bit 31 int32, bit 30 8-bit codes, else 16-bit codes on the slot bases).
// DICT: the values are 16-bit codes into the stream's dictionary (vcode: [chunk][lane][8], one 16-B load; code 0 = +0.0,
// which is also what the slots beyond a last chunk's width hold)
// FOLD (the x window in LDS): a periodic chunk leaves the lane's own part of its columns, 3 (row div 3 - first), in `loff`
// instead of adding it to each of the eight: the caller adds it to the window's address once.
template <bool NT, bool FULL, int DICT = 0, bool FOLD = false>
__device__ inline void read_chunk(int c, int w, int lane, const double* __restrict__ svals, const uint16_t* __restrict__ c16,
                                  const int32_t* __restrict__ c32, const int32_t* __restrict__ meta, dbl2 (&v)[4], int (&cl)[8],
                                  const uint16_t* __restrict__ vcode = nullptr, const double* __restrict__ dict = nullptr,
                                  int* __restrict__ loff = nullptr)
{
  if (FOLD)
    *loff = 0;
  const double* __restrict__ sp = svals + (size_t)c * 512;
  if (DICT == 1 || DICT == 2 || (DICT == 3 && dict != nullptr))
  {
    const uint4v q = vload<NT>(reinterpret_cast<const uint4v*>(vcode + (size_t)c * 512) + lane);
    // DICT == 2: `dict` is the workgroup's copy in LDS (a small dictionary: the lanes of a slice mostly hold the same
    // code in a slot -- broadcast reads); DICT == 1: gathers from memory; DICT == 3: the slice's own table in the
    // wavefront's LDS (dict == nullptr: this slice stays doubles, below)
    auto look = [&](unsigned code) -> double { return DICT == 1 ? gather(dict, (int)code) : dict[code]; };
    v[0].x = look(q.x & 0xffffu);
    v[0].y = look(q.x >> 16);
    v[1].x = look(q.y & 0xffffu);
    v[1].y = look(q.y >> 16);
    v[2].x = look(q.z & 0xffffu);
    v[2].y = look(q.z >> 16);
    v[3].x = look(q.w & 0xffffu);
    v[3].y = look(q.w >> 16);
  }
  else
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    if (FULL || 2 * j + 1 < w)
      v[j] = vload<NT>(reinterpret_cast<const dbl2*>(sp + 128 * j) + lane);
    else if (2 * j < w)
    {
      v[j].x = vload<NT>(sp + 128 * j + lane);
      v[j].y = 0.0;
    }
    else
    {
      v[j].x = 0.0;
      v[j].y = 0.0;
    }
  }
  const int32_t* __restrict__ mp = meta + (size_t)c * 8;
  const int m0 = mp[0];
  if (m0 < 0 && (m0 & 0x40000000))
  {
    // periodic chunk (block size 3): column = T[slot][row mod 3] + 3 (row div 3 - first), nothing per lane to load
    const int32_t* __restrict__ tp = reinterpret_cast<const int32_t*>(c16 + (size_t)c * 512);
    // (round 5 probe: with every chunk reading the table of one of eight chunks -- scalar-cache hits -- C4's product takes the
    // same 123-124 us: it does not wait for these loads)
    // the 25 words are wave-uniform: pinned into scalar registers, the selects below stay register selects.  (Left to
    // itself the compiler folds them into a per-lane ADDRESS select, tp + 3 e + k, behind divergent branches -- and
    // that code decoded slot 0 of the third class wrongly when the chunk sits inside the chunk loop.)
    // (All 25 requested first, pinned after: pinning each word as it is loaded made 25 DEPENDENT scalar round trips of
    // them -- `s_load_dword; s_waitcnt lgkmcnt(0)` 25 times per periodic chunk, 2-3 us of a 3.5-us chunk at C4.)
    int t[25];
#pragma unroll
    for (int i = 0; i < 25; ++i)
      t[i] = tp[i];
#pragma unroll
    for (int i = 0; i < 25; ++i)
      asm volatile("" : "+s"(t[i]));
    const int l = lane + t[24];
    const int q = l / 3, k = l - 3 * q, q3 = 3 * q;
    // T[slot][k] without a select per class: T0 + (k >= 1) (T1 - T0) + (k == 2) (T2 - T1), the brackets as masks.  (The nested
    // selects compiled into divergent control flow, ~15 scalar instructions per slot: 163 scalar instructions per chunk at C4,
    // more than the CU's scalar unit issues in the time the chunk's bytes take.)
    int k1 = k >= 1 ? -1 : 0, k2 = k == 2 ? -1 : 0;
    // (the masks made opaque: left visible, the compiler turns `mask & scalar` back into a select, which needs the scalar
    // in a vector register first -- two moves, two selects and two adds per slot; this way it is two `v_and` with a scalar
    // operand and one three-operand add: 48 -> 24 vector instructions per periodic chunk, a quarter of all it issues at C4)
    asm volatile("" : "+v"(k1), "+v"(k2));
    if (FOLD)
      *loff = q3;
#pragma unroll
    for (int e = 0; e < 8; ++e)
    {
      const int a = k1 & (t[3 * e + 1] - t[3 * e]), b = k2 & (t[3 * e + 2] - t[3 * e + 1]);
      cl[e] = FOLD ? (t[3 * e] + a) + b : ((t[3 * e] + q3) + a) + b;
    }
  }
  else if (m0 < 0)
  {
    const int4v* __restrict__ cp = reinterpret_cast<const int4v*>(c32 + (size_t)c * 512) + 2 * lane;
    const int4v q0 = vload<NT>(cp), q1 = vload<NT>(cp + 1);
    cl[0] = q0.x, cl[1] = q0.y, cl[2] = q0.z, cl[3] = q0.w;
    cl[4] = q1.x, cl[5] = q1.y, cl[6] = q1.z, cl[7] = q1.w;
  }
  else if ((m0 & 0x60000000) == 0x20000000)
  {
    // affine chunk: column = slot base + lane, nothing to load
    cl[0] = (m0 & 0x1fffffff) + lane;
#pragma unroll
    for (int e = 1; e < 8; ++e)
      cl[e] = mp[e] + lane;
  }
  else if (m0 & 0x40000000)
  {
    const uint2v q = (m0 & 0x20000000) ? vload<NT>(reinterpret_cast<const uint2v*>(sp + 448) + lane)
                                       : vload<NT>(reinterpret_cast<const uint2v*>(c16 + (size_t)c * 512) + lane);
    cl[0] = (m0 & 0x1fffffff) + (int)(q.x & 0xffu);
    cl[1] = mp[1] + (int)((q.x >> 8) & 0xffu);
    cl[2] = mp[2] + (int)((q.x >> 16) & 0xffu);
    cl[3] = mp[3] + (int)(q.x >> 24);
    cl[4] = mp[4] + (int)(q.y & 0xffu);
    cl[5] = mp[5] + (int)((q.y >> 8) & 0xffu);
    cl[6] = mp[6] + (int)((q.y >> 16) & 0xffu);
    cl[7] = mp[7] + (int)(q.y >> 24);
  }
  else
  {
    const uint4v q = vload<NT>(reinterpret_cast<const uint4v*>(c16 + (size_t)c * 512) + lane);
    cl[0] = m0 + (int)(q.x & 0xffffu);
    cl[1] = mp[1] + (int)(q.x >> 16);
    cl[2] = mp[2] + (int)(q.y & 0xffffu);
    cl[3] = mp[3] + (int)(q.y >> 16);
    cl[4] = mp[4] + (int)(q.z & 0xffffu);
    cl[5] = mp[5] + (int)(q.z >> 16);
    cl[6] = mp[6] + (int)(q.w & 0xffffu);
    cl[7] = mp[7] + (int)(q.w >> 16);
  }
}

// sum += the chunk's products in ascending column order, mul and add rounded separately (the scalar CPU loop's bits)
template <bool NT, bool FULL, bool LDS = false, int DICT = 0>
__device__ inline void chunk_product(int c, int w, int lane, const double* __restrict__ svals, const uint16_t* __restrict__ c16,
                                     const int32_t* __restrict__ c32, const int32_t* __restrict__ meta,
                                     const double* __restrict__ x, double& sum, const uint16_t* __restrict__ vcode = nullptr,
                                     const double* __restrict__ dict = nullptr)
{
  dbl2 v[4];
  int cl[8];
  int loff = 0;
  read_chunk<NT, FULL, DICT, LDS>(c, w, lane, svals, c16, c32, meta, v, cl, vcode, dict, &loff);
  const double* __restrict__ xl = LDS ? x + loff : x;
  double xv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    xv[e] = (FULL || e < w) ? (LDS ? xl[cl[e]] : gather(x, cl[e])) : 0.0; // LDS: x is the group's window, cl its index
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (FULL || e < w)
      sum += ((e & 1) ? v[e >> 1].y : v[e >> 1].x) * xv[e];
}

template <bool DOT, bool NT, bool PERM, bool CHEB = false, bool WIN = false, int DICT = 0>
__global__ __launch_bounds__(SP_BLOCK, 8) void spmv_sellp_kernel(const int2* __restrict__ desc,
                                                              const double* __restrict__ svals,
                                                              const uint16_t* __restrict__ c16,
                                                              const int32_t* __restrict__ c32,
                                                              const int32_t* __restrict__ meta,
                                                              const int32_t* __restrict__ perm,
                                                              const double* __restrict__ x, double* __restrict__ y,
                                                              int nrows, int64_t nslices, double* __restrict__ partials,
                                                              const int* __restrict__ stop_flag,
                                                              const int32_t* __restrict__ group_list, int64_t nlist,
                                                              const double* __restrict__ rvec, int pstride, int nn_is_rr,
                                                              ChebEpi epi, const int2* __restrict__ win_info,
                                                              const int2* __restrict__ win_seg, const uint16_t* __restrict__ vcode,
                                                              const double* __restrict__ dict_g, int dict_n,
                                                              const int32_t* __restrict__ sd_info,
                                                              const int64_t* __restrict__ sd_off)
{
  // dynamic LDS: DICT == 2: the value dictionary (dict_n doubles, rounded up to 2); WIN: the group's x window behind it
  // (launch: sp_win_max doubles)
  extern __shared__ __attribute__((aligned(16))) double sp_lds[];
  double* const xwin = sp_lds + (DICT == 2 ? ((dict_n + 1) & ~1) : 0);
  // DICT == 3: dict_g holds the slices' tables (SD_MAX entries each), sp_lds one table per wavefront
  double* const sdl = sp_lds + (threadIdx.x >> 6) * SD_MAX;
  const double* dict = DICT == 2 ? sp_lds : dict_g;
  // group_list != nullptr: only the listed groups of 4 slices (interior or boundary subset of a partitioned
  // matrix); rvec != nullptr: also the partials of <r,x> and of the test norm (single-reduction CG), as in
  // spmv_tile_kernel
  __shared__ double red[SP_BLOCK / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ngroups = group_list ? nlist : (nslices + 3) / 4; // a workgroup takes 4 consecutive slices
  RowSums S;
  // A slice is a chain of dependent round trips: (group list ->) descriptor -> values / codes / bases -> gathers.  At the
  // 8-GPU per-rank size a wavefront has two or three slices in all, so the kernel's length is that chain times three;
  // the slice number and descriptor of the NEXT slice are therefore requested (scalar loads) before the current slice's
  // chunks, and those of the first slice before the stop word is looked at.
  auto next_slice = [&](int i, int& s_out, int2& ds_out) -> int { // 1 valid, 0 no slice for this wavefront, -1 done
    const int64_t gi = xcd_stride_item(ngroups, i);
    if (gi < 0)
      return -1;
    const int64_t g = group_list ? group_list[gi] : gi;
    const int s = __builtin_amdgcn_readfirstlane((int)(4 * g + wv));
    s_out = s;
    if (s >= nslices)
      return 0;
    ds_out = desc[s];
    return 1;
  };
  int s_n = 0;
  int2 ds_n = make_int2(0, 0);
  int st_n = next_slice(0, s_n, ds_n);
  if (stop_flag && *stop_flag) // CG already converged: the host is a few iterations ahead
    return;
  if (DICT == 2)
  {
    // the dictionary into LDS: every thread's (at most eight) entries requested together, one round trip (five dependent ones
    // at C2's 1 204 values cost the 8-GPU per-rank product ~2 of its 12 us)
    double t[SP_DICT_LDS_ENTRIES / SP_BLOCK];
#pragma unroll
    for (int i = 0; i < SP_DICT_LDS_ENTRIES / SP_BLOCK; ++i)
    {
      const int k = (int)threadIdx.x + i * SP_BLOCK;
      t[i] = k < dict_n ? dict_g[k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < SP_DICT_LDS_ENTRIES / SP_BLOCK; ++i)
    {
      const int k = (int)threadIdx.x + i * SP_BLOCK;
      if (k < dict_n)
        sp_lds[k] = t[i];
    }
    __syncthreads();
  }
  for (int i = 0; st_n >= 0; ++i)
  {
    const int st = st_n, s = s_n;
    const int2 ds = ds_n;
    st_n = next_slice(i + 1, s_n, ds_n);
    // WIN: the four wavefronts work on one group; where the group has a window its segments of x are loaded into LDS
    // first (every wavefront takes part, also one without a slice of its own at the end of the matrix)
    int nwin = 0;
    if (WIN)
    {
      const int2 wi = win_info[s >> 2];
      nwin = __builtin_amdgcn_readfirstlane(wi.x);
      if (nwin > 0)
      {
        const int2* __restrict__ sg = win_seg + (int64_t)(s >> 2) * SP_WIN_NSEG;
        __syncthreads(); // the previous group's window is done with
        // Every entry of the window is REQUESTED before any is stored (a loop of load -> store per segment was five to
        // seven dependent round trips per group, a quarter of the group's time at C4): the segments are cut into blocks of
        // 256 entries, block i is thread-uniformly one segment's, thread t takes entry t of each; at most WIN_BLOCKS blocks
        // in registers at a time.
        constexpr int WIN_BLOCKS = 12;
        int q = 0, seg_first = 0, off = 0; // the segment of the current block, the first block of it, where it starts in the window
        int2 sq = sg[0];
        int c0s = __builtin_amdgcn_readfirstlane(sq.x), len = __builtin_amdgcn_readfirstlane(sq.y);
        for (int b0 = 0; q < nwin; b0 += WIN_BLOCKS)
        {
          double t[WIN_BLOCKS];
          int at[WIN_BLOCKS]; // where the entry goes (-1: none)
#pragma unroll
          for (int i = 0; i < WIN_BLOCKS; ++i)
          {
            at[i] = -1;
            t[i] = 0.0;
            while (q < nwin && (b0 + i - seg_first) * SP_BLOCK >= len) // (uniform: on to the segment this block belongs to)
            {
              off += len;
              seg_first = b0 + i;
              ++q;
              if (q < nwin)
              {
                sq = sg[q];
                c0s = __builtin_amdgcn_readfirstlane(sq.x);
                len = __builtin_amdgcn_readfirstlane(sq.y);
              }
            }
            if (q < nwin)
            {
              const int k = (b0 + i - seg_first) * SP_BLOCK + (int)threadIdx.x;
              if (k < len)
              {
                t[i] = x[c0s + k];
                at[i] = off + k;
              }
            }
          }
#pragma unroll
          for (int i = 0; i < WIN_BLOCKS; ++i)
            if (at[i] >= 0)
              xwin[at[i]] = t[i];
        }
        __syncthreads();
      }
    }
    if (st == 0)
      continue;
    if (DICT == 3)
    {
      // the slice's table into the wavefront's LDS (entries 0 .. n - 1; n == 0: the slice's values are doubles)
      const int n_sd = __builtin_amdgcn_readfirstlane(sd_info[s]);
      const int64_t sd_tab = sd_off[s];
      if (n_sd > 0)
      {
        __builtin_amdgcn_wave_barrier(); // (the previous slice's lookups are done)
        // the table requested 512 entries at a time before any of them is stored, 16 B per lane and request (the tables start
        // at even entries) -- not one dependent round trip per 64 entries (five for a median table of 296)
        const dbl2* __restrict__ tsrc = reinterpret_cast<const dbl2*>(dict_g + sd_tab);
        const int n2 = (n_sd + 1) >> 1;
        for (int b0 = 0; b0 * 64 < n2; b0 += 4) // (four requests = 512 entries at a time: registers)
        {
          dbl2 t[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            t[i] = lane + 64 * (b0 + i) < n2 ? tsrc[lane + 64 * (b0 + i)] : dbl2{0.0, 0.0};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (lane + 64 * (b0 + i) < n2)
              reinterpret_cast<dbl2*>(sdl)[lane + 64 * (b0 + i)] = t[i];
        }
        __builtin_amdgcn_wave_barrier();
        dict = sdl;
      }
      else
        dict = nullptr;
    }
    const int c0 = ds.x, nch = ds.y & 0xffffff, wl = ds.y >> 24;
    int r = PERM ? perm[(int64_t)s * 64 + lane] : s * 64 + lane;
    if (!PERM && r >= nrows)
      r = -1;
    const double xr = ((DOT || CHEB) && r >= 0) ? x[r] : 0.0;
    double sum = 0.0;
    if (WIN && nwin > 0)
    {
      for (int j = 0; j + 1 < nch; ++j)
        chunk_product<NT, true, true, DICT>(c0 + j, 8, lane, svals, c16, c32, meta, xwin, sum, vcode, dict);
      if (nch)
      {
        if (wl == 8)
          chunk_product<NT, true, true, DICT>(c0 + nch - 1, 8, lane, svals, c16, c32, meta, xwin, sum, vcode, dict);
        else
          chunk_product<NT, false, true, DICT>(c0 + nch - 1, wl, lane, svals, c16, c32, meta, xwin, sum, vcode, dict);
      }
    }
    else
    {
      for (int j = 0; j + 1 < nch; ++j)
        chunk_product<NT, true, false, DICT>(c0 + j, 8, lane, svals, c16, c32, meta, x, sum, vcode, dict);
      if (nch)
      {
        if (wl == 8)
          chunk_product<NT, true, false, DICT>(c0 + nch - 1, 8, lane, svals, c16, c32, meta, x, sum, vcode, dict);
        else
          chunk_product<NT, false, false, DICT>(c0 + nch - 1, wl, lane, svals, c16, c32, meta, x, sum, vcode, dict);
      }
    }
    if (CHEB)
    {
      if (r >= 0)
        cheb_row<DOT>(S, epi, nn_is_rr, r, sum, xr, y);
    }
    else if (r >= 0)
    {
      y[r] = sum;
      if (DOT)
        row_sums(S, rvec != nullptr, nn_is_rr, sum, xr, [&] { return rvec[r]; });
    }
  }
  // row_sums_store's text, kept here by hand: behind the helper this kernel's scalar registers are allocated differently and
  // the instantiations on dictionaries spill up to ten more of them
  if (DOT)
  {
    const double sres = CHEB ? 0.0 : block_reduce_sum(S.dot, red);
    double s1 = 0.0, s2 = 0.0;
    if (rvec || CHEB)
    {
      s1 = block_reduce_sum(S.dot_rx, red);
      s2 = block_reduce_sum(S.dot_nn, red);
    }
    if (threadIdx.x == 0)
    {
      if (!CHEB)
        partials[blockIdx.x] = sres;
      if (rvec || CHEB)
      {
        partials[pstride + blockIdx.x] = s1;
        partials[2 * pstride + blockIdx.x] = s2;
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------
// A failed build leaves its form off (and the stream, where there is one, as it is).
bool sellp_special_build(zzz_ctx* ctx)
{
  if (sellp_blk_build(ctx) != ZZZ_OK)
  {
    ctx->values.bk_on = false;
    (void)hipGetLastError();
  }
  if (sellp_win_build(ctx) != ZZZ_OK)
  {
    ctx->values.bw_on = false;
    (void)hipGetLastError();
  }
  return sellp_blk_serves(ctx) || sellp_win_serves(ctx);
}

bool sellp_active(zzz_ctx* ctx)
{
  if (ctx->values.sp_pending)
    (void)sellp_resolve(ctx);
  if (!ctx->values.have_sell)
    return false;
  if (!(ctx->spmv_auto || (ctx->spmv_variant & 8) != 0))
    return false;
  if (!ctx->values.sp_dict_done)
  {
    // a FAILED build (a hipMalloc that did not fit) leaves the stream on doubles -- valid -- but must not leave its partial
    // allocations or HIP's sticky last error behind (the next hipGetLastError after a product launch would report it).
    // A build that was DECLINED (too many distinct values, the 60 % rule) keeps its buffers for the next assembly: this runs
    // at the first product of a solve, and hipFree waits for the whole device -- with two ranks on ONE GPU (the tests' and
    // the driver's --comm local) the other rank may already be polling its all-reduce mailbox for this one: a release here
    // was a dead wait until the poll's time-out (round 5, found by tools/soak_driver.sh: elasticity P2, two ranks).
    // The special forms first (block rows for block size 3, zzz_sellp_blk.hip; block windows for long scalar rows,
    // zzz_sellp_win.hip): where one of them serves the product, the stream's value dictionaries are not built -- the launches
    // that still take the generic kernel read its values as doubles.  7.6 ms per assembly at 6.2 M rows of P3, 3 ms at C4.
    // A failed build leaves the stream as it is.
    ctx->values.sp_dict_done = true;
    ctx->values.sp_dict_on = ctx->values.sp_sd_on = ctx->values.sp_sd_all = ctx->values.sp_pal_on = false;
    ctx->sp_dict_n = 0;
    if (!ctx->values.sp_special_tried)
    {
      (void)sellp_special_build(ctx);
      ctx->values.sp_special_tried = true;
    }
    if (!sellp_blk_serves(ctx) && !sellp_win_serves(ctx))
    {
      if (sp_dict_build(ctx) != ZZZ_OK)
      {
        ctx->values.sp_dict_on = ctx->values.sp_pal_on = false;
        (void)hipGetLastError();
        ctx->sp_vcode.release();
      }
      if (sp_sd_build(ctx) != ZZZ_OK)
      {
        ctx->values.sp_sd_on = ctx->values.sp_sd_all = false;
        (void)hipGetLastError();
        ctx->sp_vcode8.release();
        ctx->sp_sd_vals.release();
        ctx->sp_sd_info.release();
        ctx->sp_sd_off.release();
      }
    }
    ctx->values.sp_pairs_ok = false;
    if (ctx->values.sp_one_chunk && ctx->values.sp_dict_on && ctx->bs == 1 && !ctx->sp_sorted)
      ctx->values.sp_pairs_ok = sellp_pairs_build(ctx) == ZZZ_OK;
  }
  return true;
}

// bytes one product reads from the stream (values or value codes + dictionary, column codes, bases; int32 chunks are not
// counted separately)
// as_codes: a packed slice counted as its 16-bit codes -- what the 200-MB size rules go by (below, cg_loop_exceeds_cache): they
// were set on that form's bytes, and the sizes either side of them keep the load policy, the coded diagonal and the deferred
// solution update they had before the packed form
int64_t sellp_stream_bytes(const zzz_ctx* ctx, bool as_codes)
{
  if (sellp_blk_serves(ctx))
    return ctx->bk_bytes; // (descriptors and table included)
  if (sellp_win_serves(ctx))
    return ctx->bw_bytes;
  // (a packed slice of the one-chunk kernel: 512 B of indices and palettes for its 1 024 B of codes)
  const int64_t packed = !as_codes && ctx->values.sp_pal_on && sellp_pipe_wgs(ctx, false) ? 512 * ctx->sp_pal_packed : 0;
  return (ctx->values.sp_sd_on ? ctx->sp_sd_bytes : (ctx->values.sp_dict_on ? ctx->sp_dict_bytes : ctx->values.sp_bytes)) + ctx->nslices * 8 - packed; // (x windows: sp_win_bytes, reported apart)
}

// Load policy of the product: non-temporal stream loads when one CG iteration (the stream and six vectors) cannot stay in
// the 256 MiB Infinity Cache anyway -- then the stream should not push the vectors' lines out; plain loads when it is
// resident.  (Until the value dictionary the stream alone decided, at 300 MB; a coded stream of 167 MB beside 480 MB of
// vectors reads 4 % faster non-temporally: 0.091 -> 0.087 ms at C2.)
static bool sp_stream_nt(const zzz_ctx* ctx)
{
  return (double)sellp_stream_bytes(ctx, true) + 48.0 * (double)(ctx->n_owned + ctx->n_ghost) * ctx->bs > 200.0e6;
}

// plain: the launch carries no Chebyshev epilogue, so the specialised kernels (one-chunk slices, block rows) may serve it;
// otherwise the generic kernel runs and keeps its eight workgroups per CU
static int sp_grid(const zzz_ctx* ctx, int64_t ngroups, bool sr, bool plain)
{
  // persistent workgroups: as many as are resident at once (a second round of a grid that is not would run on part of the chip)
  const int pw = plain ? sellp_pipe_wgs(ctx, sr) : 0;
  int64_t gs = 256 * (pw ? pw : 8); // (1024 or 1536 workgroups at the per-rank size: no faster)
  const int64_t need = (ngroups + 7) / 8 * 8;
  if (gs > need)
    gs = need;
  if (gs < 8)
    gs = 8;
  return (int)gs;
}

// The generic kernel's instantiations: [mode][load], then by the stream's layout and the form of its values.  The kernel
// takes rvec at run time, so the single-reduction form is the DOT instantiation.
enum SpLayout { SP_PLAIN, SP_SORTED, SP_WINDOWED, SP_LAYOUTS };
using SpKernel = decltype(&spmv_sellp_kernel<false, false, false>);
struct SpVariants
{
  SpKernel k[SP_LAYOUTS][4]; // [layout][DICT]
};
template <bool DOT, bool CHEB, bool NT>
constexpr SpVariants sp_variants()
{
  return {{{spmv_sellp_kernel<DOT, NT, false, CHEB, false, 0>, spmv_sellp_kernel<DOT, NT, false, CHEB, false, 1>,
            spmv_sellp_kernel<DOT, NT, false, CHEB, false, 2>, spmv_sellp_kernel<DOT, NT, false, CHEB, false, 3>},
           {spmv_sellp_kernel<DOT, NT, true, CHEB, false, 0>, spmv_sellp_kernel<DOT, NT, true, CHEB, false, 1>,
            spmv_sellp_kernel<DOT, NT, true, CHEB, false, 2>, spmv_sellp_kernel<DOT, NT, true, CHEB, false, 3>},
           // (windowed groups never read the slices' own dictionaries)
           {spmv_sellp_kernel<DOT, NT, false, CHEB, true, 0>, spmv_sellp_kernel<DOT, NT, false, CHEB, true, 1>,
            spmv_sellp_kernel<DOT, NT, false, CHEB, true, 2>, nullptr}}};
}
static const SpVariants sp_kernels[PM_COUNT][2] = {{sp_variants<true, false, true>(), sp_variants<true, false, false>()},
                                                   {sp_variants<true, false, true>(), sp_variants<true, false, false>()},
                                                   {sp_variants<false, false, true>(), sp_variants<false, false, false>()},
                                                   {sp_variants<true, true, true>(), sp_variants<true, true, false>()},
                                                   {sp_variants<false, true, true>(), sp_variants<false, true, false>()}};

static void launch_one(zzz_ctx* ctx, int grid, const ProductCall& c)
{
  // special: the caller sized the grid and chose the list for the block-row kernel (1: block size 3) or the block-window kernel
  // (2: long scalar rows)
  if (c.special == 1 && launch_sellp_blk(ctx, grid, c))
    return;
  if (c.special == 2 && launch_sellp_win(ctx, grid, c))
    return;
  if (launch_sellp_pipe(ctx, grid, c))
    return;
  // windowed groups: their codes index the LDS window the kernel loads per group
  const SpLayout layout = ctx->sp_sorted ? SP_SORTED : ctx->values.sp_win_max > 0 ? SP_WINDOWED : SP_PLAIN;
  size_t lds = layout == SP_WINDOWED ? (size_t)ctx->values.sp_win_max * sizeof(double) : 0;
  // the values: 3 the slices' own dictionaries, 2 the stream's dictionary in LDS, 1 the same in memory, 0 doubles
  int dict = 0;
  if (ctx->values.sp_sd_on && layout != SP_WINDOWED)
  {
    dict = 3;
    lds = (size_t)4 * SD_MAX * sizeof(double);
  }
  else if (ctx->values.sp_dict_on && ctx->sp_dict_n <= SP_DICT_LDS_ENTRIES)
  {
    dict = 2;
    lds += (size_t)((ctx->sp_dict_n + 1) & ~1) * sizeof(double);
  }
  else if (ctx->values.sp_dict_on)
    dict = 1;
  hipLaunchKernelGGL(sp_kernels[c.mode][c.load].k[layout][dict], dim3(grid), dim3(SP_BLOCK), lds, ctx->stream,
                     reinterpret_cast<const int2*>(ctx->sp_desc.p), ctx->sp_vals.p, ctx->sp_codes16.p, ctx->sp_codes32.p,
                     ctx->sp_meta.p, ctx->sp_perm.p, c.x, c.y, (int)ctx->nrows, ctx->nslices, c.partials, c.stop, c.list, c.nlist,
                     c.rvec, SPMV_PSTRIDE, c.nn_is_rr, c.epi ? *c.epi : ChebEpi(), reinterpret_cast<const int2*>(ctx->sp_win_info.p),
                     reinterpret_cast<const int2*>(ctx->sp_win_seg.p), dict == 3 ? ctx->sp_vcode8.p : ctx->sp_vcode.p,
                     dict == 3 ? ctx->sp_sd_vals.p : ctx->sp_dset.dict.p, ctx->sp_dict_n, ctx->sp_sd_info.p, ctx->sp_sd_off.p);
}

// what both drivers decide once per product: the special form that serves it (the special forms carry the Chebyshev
// epilogue; a partitioned product needs the form's own interior / boundary lists) and the load policy
static int sp_prepare(zzz_ctx* ctx, ProductCall& c, bool split)
{
  c.special = (sellp_blk_serves(ctx) && (!split || ctx->pattern.bk_have_split)) ? 1
              : (sellp_win_serves(ctx) && (!split || ctx->pattern.bw_have_split)) ? 2 : 0;
  // load policy by stream size, as for the tile kernel: a stream that stays in the 256 MiB Infinity Cache from
  // one CG iteration to the next is read with plain loads, a larger one with non-temporal loads
  bool nt = sp_stream_nt(ctx);
  if (!ctx->spmv_auto)
    nt = (ctx->spmv_variant & 1) != 0;
  c.load = nt ? LOAD_NT : LOAD_PLAIN;
  return c.special ? ZZZ_OK : sellp_need_generic(ctx);
}

int launch_sellp(zzz_ctx* ctx, ProductCall c, int* npartials)
{
  if (int rc = sp_prepare(ctx, c, false))
    return rc;
  const int gs = c.special == 1 ? sellp_blk_grid(ctx, ctx->bk_slices) : c.special == 2 ? sellp_win_grid(ctx, ctx->bw_nblk)
                 : sp_grid(ctx, (ctx->nslices + 3) / 4, c.mode == PM_DOT_SR, !c.epi);
  launch_one(ctx, gs, c);
  if (c.partials && npartials)
    *npartials = gs;
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

// Partitioned matrix: forward halo of x overlapped with the groups that reference no ghost column
// (scheme and the 7-of-8 workgroup slots: launch_overlapped in zzz_spmv.hip)
int launch_sellp_overlapped(zzz_ctx* ctx, double* x, ProductCall c, int* npartials)
{
  if (int rc = sp_prepare(ctx, c, true))
    return rc;
  const int blk = c.special;
  const bool plain = !c.epi, sr = c.mode == PM_DOT_SR;
  const int64_t gi = blk == 1 ? ctx->bk_n_interior : blk == 2 ? ctx->bw_n_interior : ctx->n_groups_interior;
  const int64_t gb = blk == 1 ? ctx->bk_n_boundary : blk == 2 ? ctx->bw_n_boundary : ctx->n_groups_boundary;
  const int32_t* list_in = blk == 1 ? ctx->bk_list_interior.p : blk == 2 ? ctx->bw_list_interior.p : ctx->groups_interior.p;
  const int32_t* list_bd = blk == 1 ? ctx->bk_list_boundary.p : blk == 2 ? ctx->bw_list_boundary.p : ctx->groups_boundary.p;
  auto grid = [&](int64_t items) {
    return !items ? 0 : blk == 1 ? sellp_blk_grid(ctx, items) : blk == 2 ? sellp_win_grid(ctx, items) : sp_grid(ctx, items, sr, plain);
  };
  int g_in = grid(gi);
  const int pw = plain ? sellp_pipe_wgs(ctx, sr) : 0;
  const int room = 256 * ((pw ? pw : 8) - 1); // (one workgroup slot per CU left to the exchange's kernel; the block-row
  if (!blk && g_in > room && ctx->nneigh > 0) //  kernel's one workgroup per CU leaves half the CU's wavefront slots free)
    g_in = room;
  const int g_bd = grid(gb);
  if (c.partials && (size_t)(g_in + g_bd) > (size_t)SPMV_PSTRIDE)
    return fail(ctx, ZZZ_ERR_ARG, "partials buffer too small");
  return launch_overlapped(ctx, x, c, {gi, list_in, g_in}, {gb, list_bd, g_bd}, launch_one, npartials);
}
ZZZ_PRELOAD_TU(sellp)
} // namespace zzz
