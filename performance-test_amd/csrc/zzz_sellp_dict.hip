// The CG operator stream, part 2 of 3: the VALUE DICTIONARIES of a packed stream (matrix-wide, copied into LDS by the product's
// workgroups; per slice for long rows).  Packer: zzz_sellp_pack.hip; product: zzz_sellp.hip / zzz_sellp_pipe.hip.
#include <climits>
#include <cstring>
#include <cstdlib>

#include "zzz_sellp.h"

#include "zzz_prim.h"

namespace zzz
{
struct Even2
{
  __host__ __device__ int64_t operator()(int32_t n) const { return ((int64_t)n + 1) & ~(int64_t)1; }
};
// ---- value dictionary -----------------------------------------------------------------------------------
// The entries of the packed stream as (slice, chunk, lane, slot) with the values the product would load: slots of a
// slice's last chunk beyond its width and lanes without a row are never loaded (and hold anything).
constexpr int SP_DICT_BITS = decltype(zzz_ctx::sp_dset)::bits; // table of 2^18 slots (zzz_valset.h)
constexpr int SP_DICT_MAX = 65535;

// value of entry (chunk c of width w, lane, slot e) in the value blocks: [4][64 lanes][2]; the last entry of an odd width
// sits alone, 8 B per lane (emit_chunk)
__device__ inline unsigned long long sp_value_bits(const double* __restrict__ svals, int64_t c, int w, int lane, int e)
{
  const int64_t at = ((w & 1) && e == w - 1) ? 128 * (e >> 1) + lane : 128 * (e >> 1) + 2 * lane + (e & 1);
  return reinterpret_cast<const unsigned long long*>(svals)[c * 512 + at];
}

// the stream's distinct values into the set (zzz_valset.h); a lane skips the value it has just seen
template <bool PERM>
__global__ __launch_bounds__(256) void k_sp_dict_insert(const int2* __restrict__ desc, const int32_t* __restrict__ perm,
                                                         const double* __restrict__ svals, int nrows, int64_t nslices,
                                                         unsigned long long* __restrict__ table, int* __restrict__ info, int limit)
{
  const int lane = threadIdx.x & 63;
  for (int64_t s = blockIdx.x * 4ll + (threadIdx.x >> 6); s < nslices; s += gridDim.x * 4ll)
  {
    const int r = PERM ? perm[s * 64 + lane] : (int)(s * 64 + lane);
    const bool row = r >= 0 && r < nrows;
    const int2 ds = desc[s];
    const int c0 = ds.x, nch = ds.y & 0xffffff, wl = ds.y >> 24;
    unsigned long long last = 0ull; // (+0.0 is code 0 without the table)
    for (int j = 0; j < nch; ++j)
    {
      const int w = j + 1 < nch ? 8 : wl;
      for (int e = 0; e < w; ++e)
      {
        const unsigned long long b = row ? sp_value_bits(svals, c0 + j, w, lane, e) : 0ull;
        const bool need = b != last && b != 0ull; // (a row repeats its values: the previous one is in the table already)
        last = b;
        if (!valset_insert_wave<SP_DICT_BITS>(table, info, limit, b, need))
          return; // more distinct values than the dictionary may hold (an unstructured mesh): nothing left to find out
      }
    }
  }
}

// the stream's values as codes, [chunk][lane][8] (16 B per lane and chunk); bytes_out: bytes the product reads in this form
template <bool PERM>
__global__ __launch_bounds__(256) void k_sp_dict_encode(const int2* __restrict__ desc, const int32_t* __restrict__ perm,
                                                         const double* __restrict__ svals, const int32_t* __restrict__ meta,
                                                         int nrows, int64_t nslices, const unsigned long long* __restrict__ table,
                                                         const int32_t* __restrict__ slot_code, const int* __restrict__ info,
                                                         uint16_t* __restrict__ vcode, unsigned long long* __restrict__ bytes_out)
{
  if (info[1])
    return;
  const int lane = threadIdx.x & 63;
  unsigned long long bytes = 0;
  for (int64_t s = blockIdx.x * 4ll + (threadIdx.x >> 6); s < nslices; s += gridDim.x * 4ll)
  {
    const int r = PERM ? perm[s * 64 + lane] : (int)(s * 64 + lane);
    const bool row = r >= 0 && r < nrows;
    const int2 ds = desc[s];
    const int c0 = ds.x, nch = ds.y & 0xffffff, wl = ds.y >> 24;
    unsigned long long last = 0ull;
    unsigned last_code = 0;
    for (int j = 0; j < nch; ++j)
    {
      const int w = j + 1 < nch ? 8 : wl;
      unsigned code[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
      {
        code[e] = 0;
        if (row && e < w)
        {
          const unsigned long long b = sp_value_bits(svals, c0 + j, w, lane, e);
          if (b == 0ull)
            continue;
          if (b != last)
          {
            last = b;
            last_code = (unsigned)valset_find<SP_DICT_BITS>(table, slot_code, b);
          }
          code[e] = last_code;
        }
      }
      uint4v q;
      q.x = code[0] | (code[1] << 16);
      q.y = code[2] | (code[3] << 16);
      q.z = code[4] | (code[5] << 16);
      q.w = code[6] | (code[7] << 16);
      reinterpret_cast<uint4v*>(vcode + (size_t)(c0 + j) * 512)[lane] = q;
      if (lane == 0)
      {
        // what the product reads of this chunk: 1 KiB of value codes, the slot bases, the column codes by the chunk's mode
        const int m0 = meta[(size_t)(c0 + j) * 8];
        unsigned cb = 0;
        if (m0 < 0 && (m0 & 0x40000000))
          cb = 100; // periodic: 25 scalar words
        else if (m0 < 0)
          cb = 2048; // int32 columns
        else if ((m0 & 0x60000000) == 0x20000000)
          cb = 0; // affine
        else if (m0 & 0x40000000)
          cb = 512; // 8-bit codes
        else
          cb = 1024; // 16-bit codes
        bytes += 1024 + 32 + cb;
      }
    }
  }
  if (lane == 0 && bytes)
    atomicAdd(bytes_out, bytes);
}

// ---- the packed form of one-chunk slices: 4-bit palette indices --------------------------------------------------------
// The 1 200 values of a regular mesh's matrix are rounding variants of a handful of stencil entries: the 64 rows of a slice
// hold three or four distinct codes in a slot, seldom more than a dozen.  One wavefront per slice, lane = row, ONE walk over
// the codes just written: per slot the distinct codes are collected (the first lane still without a palette entry names the
// next one: as many rounds as there are values), ranked, and stored ascending -- the result depends on the codes alone.  Every
// slot at most 16: the slice is PACKED -- pal[chunk][lane] = {the row's eight 4-bit indices, slot e at bits 4 e; palette codes
// 2 l and 2 l + 1 of the slice's 8 x 16} (512 B; unused palette entries: code 0), palok[slice] = 1.  Otherwise its block is
// zeros and palok[slice] = 0: the product reads its 16-bit codes.  A slot beyond the width and a lane without a row hold code 0
// like any +0.0 and count as that value.  info: [0] packed slices, [1] the largest count met, [2] mixed pairs (k_sp_pal_mixed).
__global__ __launch_bounds__(256) void k_sp_pal_build(const int2* __restrict__ desc, const uint16_t* __restrict__ vcode, int64_t nslices,
                                                       const int* __restrict__ dict_info, uint2* __restrict__ pal,
                                                       uint8_t* __restrict__ palok, int32_t* __restrict__ info)
{
  __shared__ uint16_t pal_s[4][128];
  if (dict_info[1])
    return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint16_t* const ps = pal_s[wv];
  int npacked = 0, maxc = 0;
  for (int64_t s = blockIdx.x * 4ll + wv; s < nslices; s += gridDim.x * 4ll)
  {
    const int2 ds = desc[s];
    const int nch = ds.y & 0xffffff;
    if (nch != 1) // (no chunk: nothing to read, packed or not; one-chunk streams have no longer slices)
    {
      if (lane == 0)
        palok[s] = 0;
      continue;
    }
    const uint4v q = reinterpret_cast<const uint4v*>(vcode + (size_t)ds.x * 512)[lane];
    const unsigned code[8] = {q.x & 0xffffu, q.x >> 16, q.y & 0xffffu, q.y >> 16, q.z & 0xffffu, q.z >> 16, q.w & 0xffffu, q.w >> 16};
    ps[2 * lane] = 0;
    ps[2 * lane + 1] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned idx = 0;
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 8; ++e)
    {
      const unsigned cur = code[e];
      bool rem = true;
      unsigned myval = 0, mine = 0; // lane k: the k-th value found; the lane's own value is the mine-th
      int k = 0;
      for (;;)
      {
        const unsigned long long m = __ballot(rem);
        if (!m)
          break;
        const unsigned v = (unsigned)__builtin_amdgcn_readlane((int)cur, __builtin_amdgcn_readfirstlane(__builtin_ctzll(m)));
        if (cur == v)
        {
          mine = (unsigned)k;
          rem = false;
        }
        if (lane == k)
          myval = v;
        ++k;
      }
      maxc = k > maxc ? k : maxc;
      if (k > 16)
      {
        ok = false;
        continue;
      }
      unsigned rank = 0;
      for (int j = 0; j < k; ++j)
        rank += (unsigned)__builtin_amdgcn_readlane((int)myval, j) < myval ? 1u : 0u;
      if (lane < k)
        ps[e * 16 + rank] = (uint16_t)myval;
      idx |= (unsigned)__shfl((int)rank, (int)mine) << (4 * e);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint2 out = make_uint2(0u, 0u);
    if (ok)
      out = make_uint2(idx, (unsigned)ps[2 * lane] | ((unsigned)ps[2 * lane + 1] << 16));
    pal[(size_t)ds.x * 64 + lane] = out;
    if (lane == 0)
      palok[s] = ok ? 1 : 0;
    npacked += ok ? 1 : 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0)
  {
    if (npacked)
      atomicAdd(&info[0], npacked);
    if (maxc)
      atomicMax(&info[1], maxc);
  }
}

// pairs of slices 2 p, 2 p + 1 of which one is packed and one is not (the product takes them a lane per row)
__global__ __launch_bounds__(256) void k_sp_pal_mixed(const uint8_t* __restrict__ palok, int64_t nslices, const int* __restrict__ dict_info,
                                                       int32_t* __restrict__ info)
{
  if (dict_info[1])
    return;
  int n = 0;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; 2 * p + 1 < nslices; p += (int64_t)gridDim.x * blockDim.x)
    n += palok[2 * p] != palok[2 * p + 1] ? 1 : 0;
  if (n)
    atomicAdd(&info[2], n);
}

// ---- per-slice value dictionaries (long rows: P3) ----------------------------------------------------------------
// A slice of 64 rows of one entity type holds a few hundred distinct values even where the whole matrix holds thousands
// (P3 at 30^3 sub-cubes: median 296 per slice, all slices below 1 024; 7 400 in the matrix; 8 270 at 61^3).  One wavefront
// per slice: the slice's distinct values into a hash set in LDS (at most 1 023 besides +0.0), numbered as they arrive; then
// every value of the slice as a 16-bit code in the layout of the matrix-wide dictionary's codes ([chunk][lane][8], 16 B per
// lane and chunk), and the table beside it (sd_info[slice] = entries, 0 = this slice stays doubles; the tables back to back in
// sd_vals, slice s at sd_off[s]: a first pass (COUNT) finds the sizes, a scan the offsets -- 1 024 doubles reserved per slice
// were 6.4 GB at 49.8 M rows for 1.8 GB of tables).
// The product copies a slice's table into its wavefront's part of LDS (8 KiB per wavefront: five workgroups per CU).
// Tried: 8-bit codes and tables of 256 (a third of P3's slices qualify: product 0.67 -> 0.54 ms at 6.2 M dofs), tables of 512
// (0.46 ms there, 4.19 ms at 49.8 M dofs), tables of 1 024 (0.47 / 3.68 ms: kept).
// (SD_SLOTS = 2048, SD_MAX = 1024: zzz_sellp.h; the hash: zzz_valset.h)
template <bool PERM, bool COUNT>
__global__ __launch_bounds__(128) void k_sp_sd_build(const int2* __restrict__ desc, const int32_t* __restrict__ perm,
                                                      const double* __restrict__ svals, const int32_t* __restrict__ meta,
                                                      int nrows, int64_t nslices, uint16_t* __restrict__ vcode8,
                                                      double* __restrict__ sd_vals, const int64_t* __restrict__ sd_off,
                                                      int32_t* __restrict__ sd_info, unsigned long long* __restrict__ bytes_out)
{
  __shared__ unsigned long long keys_s[2][SD_SLOTS];
  __shared__ uint16_t code_s[2][SD_SLOTS];
  __shared__ int cnt_s[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long* const keys = keys_s[wv];
  uint16_t* const codes = code_s[wv];
  unsigned long long bytes = 0;
  for (int64_t s = blockIdx.x * 2ll + wv; s < nslices; s += gridDim.x * 2ll)
  {
    for (int k = lane; k < SD_SLOTS; k += 64)
      keys[k] = ~0ull;
    if (lane == 0)
      cnt_s[wv] = 1; // (entry 0 is +0.0)
    __builtin_amdgcn_wave_barrier();
    const int r = PERM ? perm[s * 64 + lane] : (int)(s * 64 + lane);
    const bool row = r >= 0 && r < nrows;
    const int2 ds = desc[s];
    const int c0 = ds.x, nch = ds.y & 0xffffff, wl = ds.y >> 24;
    if (!COUNT && sd_info[s] == 0) // (the first pass found more values than a table holds: this slice stays doubles)
    {
      if (lane == 0)
      {
        for (int j = 0; j < nch; ++j)
        {
          const int w = j + 1 < nch ? 8 : wl;
          const int m0 = meta[(size_t)(c0 + j) * 8];
          const unsigned cb = (m0 < 0 && (m0 & 0x40000000)) ? 100u : (m0 < 0 ? 2048u : ((m0 & 0x60000000) == 0x20000000 ? 0u : ((m0 & 0x40000000) ? 512u : 1024u)));
          bytes += 32 + cb + (unsigned)((w >> 1) * 1024 + (w & 1) * 512);
        }
        bytes += 4;
        atomicAdd(reinterpret_cast<int*>(bytes_out) + 2, 1); // slices that stay doubles
      }
      continue;
    }
    double* const tab = COUNT ? nullptr : sd_vals + sd_off[s];
    if (!COUNT && lane == 0)
      tab[0] = 0.0;
    unsigned long long last = 0ull;
    for (int j = 0; j < nch; ++j)
    {
      if (cnt_s[wv] > SD_MAX)
        break; // (more values than the table holds: this slice stays doubles)
      const int w = j + 1 < nch ? 8 : wl;
      for (int e = 0; e < w; ++e)
      {
        const unsigned long long b = row ? sp_value_bits(svals, c0 + j, w, lane, e) : 0ull;
        if (b != 0ull && b != last && b != ~0ull)
        {
          unsigned h = valset_hash<SD_BITS>(b);
          for (int probe = 0; probe < SD_SLOTS; ++probe)
          {
            const unsigned long long cur = keys[h];
            if (cur == b)
              break;
            if (cur == ~0ull)
            {
              const unsigned long long old = atomicCAS(&keys[h], ~0ull, b);
              if (old == ~0ull)
              {
                const int c = atomicAdd(&cnt_s[wv], 1);
                codes[h] = (uint16_t)c;
                if (!COUNT && c < SD_MAX)
                  tab[c] = __longlong_as_double((long long)b);
                break;
              }
              if (old == b)
                break;
            }
            h = (h + 1) & (SD_SLOTS - 1);
            if (cnt_s[wv] > SD_MAX)
              break;
          }
        }
        if (b == ~0ull)
          cnt_s[wv] = SD_MAX + 1;
        last = b;
      }
    }
    __builtin_amdgcn_wave_barrier();
    const int n = cnt_s[wv];
    const bool ok = n <= SD_MAX;
    if (COUNT)
    {
      if (lane == 0)
        sd_info[s] = ok ? n : 0;
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    if (ok)
    {
      last = 0ull;
      unsigned last_code = 0;
      for (int j = 0; j < nch; ++j)
      {
        const int w = j + 1 < nch ? 8 : wl;
        unsigned code[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
        {
          code[e] = 0;
          if (row && e < w)
          {
            const unsigned long long b = sp_value_bits(svals, c0 + j, w, lane, e);
            if (b == 0ull)
              continue;
            if (b != last)
            {
              unsigned h = valset_hash<SD_BITS>(b);
              while (keys[h] != b)
                h = (h + 1) & (SD_SLOTS - 1);
              last = b;
              last_code = codes[h];
            }
            code[e] = last_code;
          }
        }
        uint4v q;
        q.x = code[0] | (code[1] << 16);
        q.y = code[2] | (code[3] << 16);
        q.z = code[4] | (code[5] << 16);
        q.w = code[6] | (code[7] << 16);
        reinterpret_cast<uint4v*>(vcode8 + (size_t)(c0 + j) * 512)[lane] = q;
      }
    }
    if (lane == 0)
    {
      // what the product reads of this slice: the table and per chunk 512 B of codes, or the values as before
      for (int j = 0; j < nch; ++j)
      {
        const int w = j + 1 < nch ? 8 : wl;
        const int m0 = meta[(size_t)(c0 + j) * 8];
        unsigned cb = 0;
        if (m0 < 0 && (m0 & 0x40000000))
          cb = 100;
        else if (m0 < 0)
          cb = 2048;
        else if ((m0 & 0x60000000) == 0x20000000)
          cb = 0;
        else if (m0 & 0x40000000)
          cb = 512;
        else
          cb = 1024;
        bytes += 32 + cb + (ok ? 1024 : (unsigned)((w >> 1) * 1024 + (w & 1) * 512));
      }
      bytes += ok ? (unsigned)n * 8 + 4 : 4;
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0 && bytes)
    atomicAdd(bytes_out, bytes);
}

// ---- host side ------------------------------------------------------------------------------------------
// The value dictionary of the finished stream (see zzz_internal.h): distinct values into a hash set, numbered, every
// value of the stream replaced by its code.  Synchronous (once per assembly, at the first use of the stream): 1-2 ms at
// 10 M rows.  More than 65 535 distinct values, or ZZZ_SELLP_DICT=0: the stream keeps being read as values.
int sp_dict_build(zzz_ctx* ctx)
{
  ctx->values.sp_dict_done = true;
  ctx->values.sp_dict_on = ctx->values.sp_pal_on = false;
  ctx->sp_dict_n = 0;
  // ZZZ_SELLP_DICT: 0 never, 2 always (tests at small sizes), 1: for streams of more than 48 MB of values -- below that the
  // whole loop sits in the Infinity Cache, bytes are not what the product waits for, and building the dictionary (three
  // passes over the stream and a synchronisation, ~0.4 ms at 500 k rows) costs more than a solve gains
  if (!ctx->knob.sellp_dict || ctx->values.sp_chunks <= 0 || (ctx->knob.sellp_dict == 1 && ctx->values.sp_bytes < 48ll << 20))
    return ZZZ_OK;
  hipStream_t s = ctx->stream;
  const int64_t nsl = ctx->nslices;
  ValSet<SP_DICT_BITS, 1>& vs = ctx->sp_dset;
  ZZZ_HIP(ctx, vs.begin(SP_DICT_MAX + 1, s, ctx->retired));
  ZZZ_HIP(ctx, ctx->sp_vcode.alloc((size_t)ctx->values.sp_chunks * 512));
  ZZZ_HIP(ctx, ctx->sp_dict_info.reserve(4));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->sp_dict_info.p, 0, 4 * sizeof(int32_t), s));
  unsigned long long* bytes = reinterpret_cast<unsigned long long*>(ctx->sp_dict_info.p);
  const int2* desc = reinterpret_cast<const int2*>(ctx->sp_desc.p);
  const unsigned grid = (unsigned)std::min<int64_t>((nsl + 3) / 4, 256 * 16);
  // The search stops at the first value beyond what will be used: the LDS copy's capacity, unless the memory form is forced.
  // A dictionary too large for the LDS copy is gathered from memory: 2.3x fewer bytes at P3 6.2 M dofs (8 270 values) and the
  // same 0.61-0.63 ms per product -- the gathers, not the bytes, are what the kernel waits for -- so that form is not used
  // unless ZZZ_SELLP_DICT=2 asks for it (tests)
  const int limit = ctx->knob.sellp_dict == 2 ? SP_DICT_MAX - 1 : SP_DICT_LDS_ENTRIES - 2;
  if (ctx->sp_sorted)
    hipLaunchKernelGGL(k_sp_dict_insert<true>, dim3(grid), dim3(256), 0, s, desc, ctx->sp_perm.p, ctx->sp_vals.p, (int)ctx->nrows, nsl,
                       vs.table.p, vs.info.p, limit);
  else
    hipLaunchKernelGGL(k_sp_dict_insert<false>, dim3(grid), dim3(256), 0, s, desc, (const int32_t*)nullptr, ctx->sp_vals.p,
                       (int)ctx->nrows, nsl, vs.table.p, vs.info.p, limit);
  vs.number(s);
  if (ctx->sp_sorted)
    hipLaunchKernelGGL(k_sp_dict_encode<true>, dim3(grid), dim3(256), 0, s, desc, ctx->sp_perm.p, ctx->sp_vals.p, ctx->sp_meta.p,
                       (int)ctx->nrows, nsl, vs.table.p, vs.slot.p, vs.info.p, ctx->sp_vcode.p, bytes);
  else
    hipLaunchKernelGGL(k_sp_dict_encode<false>, dim3(grid), dim3(256), 0, s, desc, (const int32_t*)nullptr, ctx->sp_vals.p,
                       ctx->sp_meta.p, (int)ctx->nrows, nsl, vs.table.p, vs.slot.p, vs.info.p, ctx->sp_vcode.p, bytes);
  unsigned long long hb = 0;
  ZZZ_HIP(ctx, hipMemcpyAsync(&hb, bytes, sizeof(hb), hipMemcpyDeviceToHost, s));
  // the packed form of the codes (ZZZ_SELLP_PAL: 0 never, 1 default) for the streams spmv_one_kernel serves (sellp_pipe_wgs:
  // one-chunk slices, natural order, the dictionary in LDS): built behind the encoding, read back with the same synchronisation
  const bool pal = ctx->knob.sellp_pal && ctx->values.sp_one_chunk && !ctx->sp_sorted && ctx->bs == 1 && ctx->values.sp_win_max == 0;
  int32_t hp[4] = {0, 0, 0, 0};
  if (pal)
  {
    ZZZ_HIP(ctx, ctx->sp_pal.alloc((size_t)ctx->values.sp_chunks * 64));
    ZZZ_HIP(ctx, ctx->sp_palok.alloc((size_t)nsl + 1));
    ZZZ_HIP(ctx, ctx->sp_pal_info.reserve(4));
    ZZZ_HIP(ctx, hipMemsetAsync(ctx->sp_pal_info.p, 0, 4 * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_sp_pal_build, dim3(grid), dim3(256), 0, s, desc, ctx->sp_vcode.p, nsl, vs.info.p, ctx->sp_pal.p, ctx->sp_palok.p,
                       ctx->sp_pal_info.p);
    hipLaunchKernelGGL(k_sp_pal_mixed, dim3((unsigned)std::min<int64_t>((nsl / 2 + 255) / 256 + 1, 1024)), dim3(256), 0, s, ctx->sp_palok.p,
                       nsl, vs.info.p, ctx->sp_pal_info.p);
    ZZZ_HIP(ctx, hipMemcpyAsync(hp, ctx->sp_pal_info.p, sizeof(hp), hipMemcpyDeviceToHost, s));
  }
  int n = 0;
  ZZZ_HIP(ctx, vs.finish(s, n));
  if (!n)
    return ZZZ_OK;
  ctx->sp_dict_n = n;
  ctx->sp_dict_bytes = (int64_t)hb + (int64_t)n * 8;
  ctx->values.sp_dict_on = true;
  ctx->sp_pal_packed = hp[0];
  ctx->sp_pal_maxcount = hp[1];
  ctx->sp_pal_mixed = hp[2];
  ctx->values.sp_pal_on = pal && n <= SP_DICT_LDS_ENTRIES && hp[0] > 0;
  return ZZZ_OK;
}

// Per-slice dictionaries (k_sp_sd_build) for streams whose global dictionary does not fit LDS: long rows (P3).  Kept when
// they take the stream below 60 % of its bytes.  ZZZ_SELLP_DICT: 0 none of this, 3 slice dictionaries whenever they apply.
int sp_sd_build(zzz_ctx* ctx)
{
  ctx->values.sp_sd_on = ctx->values.sp_sd_all = false;
  if (!ctx->knob.sellp_dict || ctx->values.sp_dict_on || ctx->values.sp_chunks <= 0 || ctx->values.sp_win_max > 0)
    return ZZZ_OK;
  if (ctx->knob.sellp_dict != 3 && (ctx->values.sp_bytes < 48ll << 20 || ctx->values.sp_chunks < 4 * ctx->nslices))
    return ZZZ_OK; // (small streams: bytes do not matter; short rows -- P1: the table would cost as much as it saves)
  hipStream_t s = ctx->stream;
  const int64_t nsl = ctx->nslices;
  ZZZ_HIP(ctx, ctx->sp_vcode8.alloc((size_t)ctx->values.sp_chunks * 512));
  ZZZ_HIP(ctx, ctx->sp_sd_info.alloc((size_t)nsl + 1));
  ZZZ_HIP(ctx, ctx->sp_sd_off.alloc((size_t)nsl + 1));
  ZZZ_HIP(ctx, ctx->sp_dict_info.reserve(4));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->sp_dict_info.p, 0, 4 * sizeof(int32_t), s));
  ZZZ_HIP(ctx, hipMemsetAsync(ctx->sp_sd_info.p + nsl, 0, sizeof(int32_t), s)); // closes the scan
  const int2* desc = reinterpret_cast<const int2*>(ctx->sp_desc.p);
  const unsigned grid = (unsigned)std::min<int64_t>((nsl + 1) / 2, 256 * 8);
  unsigned long long* bytes = reinterpret_cast<unsigned long long*>(ctx->sp_dict_info.p);
  // first pass: the tables' sizes; scan: where each starts; second pass: tables and codes
  if (ctx->sp_sorted)
    hipLaunchKernelGGL((k_sp_sd_build<true, true>), dim3(grid), dim3(128), 0, s, desc, ctx->sp_perm.p, ctx->sp_vals.p, ctx->sp_meta.p,
                       (int)ctx->nrows, nsl, (uint16_t*)nullptr, (double*)nullptr, (const int64_t*)nullptr, ctx->sp_sd_info.p, bytes);
  else
    hipLaunchKernelGGL((k_sp_sd_build<false, true>), dim3(grid), dim3(128), 0, s, desc, (const int32_t*)nullptr, ctx->sp_vals.p,
                       ctx->sp_meta.p, (int)ctx->nrows, nsl, (uint16_t*)nullptr, (double*)nullptr, (const int64_t*)nullptr,
                       ctx->sp_sd_info.p, bytes);
  const auto even = rocprim::make_transform_iterator(ctx->sp_sd_info.p, Even2{}); // (tables start at even entries: 16-B aligned)
  if (int rc = with_scratch(ctx, scan_excl(even, ctx->sp_sd_off.p, (size_t)nsl + 1, s)))
    return rc;
  int64_t total = 0;
  ZZZ_HIP(ctx, dev_fetch(ctx, ctx->sp_sd_off.p + nsl, &total));
  ZZZ_HIP(ctx, ctx->sp_sd_vals.alloc((size_t)total + 2));
  if (ctx->sp_sorted)
    hipLaunchKernelGGL((k_sp_sd_build<true, false>), dim3(grid), dim3(128), 0, s, desc, ctx->sp_perm.p, ctx->sp_vals.p, ctx->sp_meta.p,
                       (int)ctx->nrows, nsl, ctx->sp_vcode8.p, ctx->sp_sd_vals.p, ctx->sp_sd_off.p, ctx->sp_sd_info.p, bytes);
  else
    hipLaunchKernelGGL((k_sp_sd_build<false, false>), dim3(grid), dim3(128), 0, s, desc, (const int32_t*)nullptr, ctx->sp_vals.p,
                       ctx->sp_meta.p, (int)ctx->nrows, nsl, ctx->sp_vcode8.p, ctx->sp_sd_vals.p, ctx->sp_sd_off.p, ctx->sp_sd_info.p,
                       bytes);
  ZZZ_HIP(ctx, hipGetLastError());
  int32_t h[4];
  ZZZ_HIP(ctx, hipMemcpyAsync(h, ctx->sp_dict_info.p, sizeof(h), hipMemcpyDeviceToHost, s));
  ZZZ_HIP(ctx, hipStreamSynchronize(s));
  unsigned long long b = 0;
  memcpy(&b, h, sizeof(b));
  if (ctx->knob.sellp_dict != 3 && (double)b > 0.6 * (double)ctx->values.sp_bytes)
    return ZZZ_OK;
  if ((int64_t)h[2] >= nsl)
    return ZZZ_OK; // (no slice got a dictionary: the stream is read as doubles and says so)
  ctx->sp_sd_bytes = (int64_t)b;
  ctx->values.sp_sd_on = true;
  ctx->values.sp_sd_all = h[2] == 0;
  return ZZZ_OK;
}
ZZZ_PRELOAD_TU(sellp_dict)
} // namespace zzz
