// The CG product on operator streams of ONE-CHUNK SLICES (round 5): scalar P1 on a regular mesh, BASELINE configs 2 and 3.
//
// Replaces PETSc MatMult inside KSPSolve (src/poisson_problem.cpp:177) and the `action` of linalg::cg (src/cg.h:62), like
// spmv_sellp_kernel of zzz_sellp.hip, on the same stream and with the same arithmetic (a row's products added in ascending
// column order, mul and add rounded separately: bit-identical to the serial CSR loop and to the generic kernel).
//
// What was measured before this kernel was written (MI355X, C2: 10 M rows, 156 k slices, values as 16-bit codes):
//   * the generic kernel: 0.083 ms = 0.49 of the HBM peak; its wavefronts sit in s_waitcnt 80 % of their cycles;
//   * timing probes with one kind of access after the other taken out (wrong results, time only): without the gathers of x the
//     kernel runs at 5.9 TB/s, i.e. at the speed of its bytes -- the gathers, which add no HBM bytes, cost 36 of 91 us; so do the
//     stream loads when the gathers stay; the parts ADD UP (instruction issue alone: 32 us);
//   * tools/micro/gather_rate.hip: a vector-memory instruction costs the CU's address path ~15 clk whatever it moves -- two
//     lanes or 64, 8 B or 16 B per lane, a dense run or one address 64 times; only scattered lines cost more (31 clk);
//   * variants of a lane-per-row kernel with look-ahead of one or two slices, 5 to 8 workgroups per CU, half the scalar
//     instructions, the bases through the scalar cache: each took what its COUNT of vector-memory instructions per slice
//     predicts (10.3 -> 0.080 ms, 11.3 -> 0.085, 13 -> 0.091): ~25 clk per instruction in the product's mix of hits and misses.
// So this kernel moves the same bytes in fewer instructions (below); what remains (0.074 ms at C2, 0.55 of the peak) is no
// longer explained by that count -- deeper look-ahead, a touch of the farthest run a step ahead and staggered wavefronts
// were measured and changed nothing: see DESIGN.md section 4b.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <type_traits>

#include "zzz_sellp.h"

namespace zzz
{
// what the launcher hands over beside the stream's arrays (those are __restrict__ parameters of their own: only then does the
// compiler know that the stores to y do not touch them, and reads the slot bases with scalar loads inside the loop)
struct PipeArgs
{
  int dict_n;
  int nrows;
  int nslices;
  double* partials;
  const int* stop_flag;
  int64_t nlist;
  int pstride, nn_is_rr;
};

// TWO slices per wavefront and step, a lane owning rows 2 l and 2 l + 1 of the 128: where both slices are affine with the same
// slot layout (slot e of the second starts 64 columns behind slot e of the first: an interior slice pair of a regular mesh --
// 99.4 % of the pairs at C2; found once per packing, k_sp_pairs) slot e of the pair is ONE run of 128 doubles, i.e. one 16-B
// load per lane instead of two gathers; x of the own rows and the store are one 16-B access each; the codes of a lane's two
// rows are 32 contiguous bytes of one of the two chunks.  Eleven vector-memory instructions per 128 rows instead of twenty-one.
// A pair that does not qualify (a slice with column codes, another width, the last slice of an odd count) takes its two slices
// one after the other in the lane-per-row form.  Slot bases come through the scalar cache (no vector instruction), a slice's
// column codes are loaded only where it has any, a slot beyond the width costs nothing.  One stage of look-ahead: the next
// step's value codes and bases are requested behind this step's gathers (vmcnt retires in order: behind them, so that the
// products wait for the gathers alone); the two stages are two named register sets and the loop body exists twice -- no
// register that a load is still writing is ever copied.  What a wavefront will meet is known without a memory round trip: the
// descriptors and mode words (zzz_sellp.h) of its next 64 steps sit in three vector registers, lane i = step i.
typedef double dbl2u __attribute__((ext_vector_type(2), aligned(8))); // a 16-B load from an 8-B aligned address

// pairs[p] = 1: slices 2 p and 2 p + 1 form an affine pair (see above)
__global__ __launch_bounds__(256) void k_sp_pairs(const int2* __restrict__ desc, const unsigned long long* __restrict__ smode,
                                                  const int32_t* __restrict__ meta, int64_t nslices, uint8_t* __restrict__ pairs)
{
  const int64_t npairs = (nslices + 1) / 2;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * blockDim.x)
  {
    bool ok = 2 * p + 1 < nslices;
    if (ok)
    {
      const int2 da = desc[2 * p], db = desc[2 * p + 1];
      ok = (da.y & 0xffffff) == 1 && (db.y & 0xffffff) == 1 && (da.y >> 24) == (db.y >> 24) && (smode[2 * p] & 3ull) == 0ull
           && (smode[2 * p + 1] & 3ull) == 0ull;
      if (ok)
      {
        const int32_t* ma = meta + (int64_t)da.x * 8;
        const int32_t* mb = meta + (int64_t)db.x * 8;
        const int w = da.y >> 24;
        ok = ma[0] >= 0 && mb[0] >= 0 && (ma[0] & 0x60000000) == 0x20000000 && (mb[0] & 0x60000000) == 0x20000000; // affine, both
        for (int e = 0; e < w && ok; ++e)
        {
          const int ba = e ? ma[e] : (ma[0] & 0x1fffffff), bb = e ? mb[e] : (mb[0] & 0x1fffffff);
          ok = bb - ba == 64;
        }
      }
    }
    pairs[p] = ok ? 1 : 0;
  }
}

// PAL: the PACKED form of the value codes (k_sp_pal_build, zzz_sellp_dict.hip; the layout: zzz_internal.h, sp_pal).  A slice
// whose every slot holds at most 16 distinct codes is read as 512 B instead of 1 024: per row eight 4-bit indices into the
// slice's palettes (8 slots x 16 codes).  An affine pair of two packed slices takes its stream in ONE 16-B load per lane (lanes
// 0..31 the first slice's block, 32..63 the second's): the lane's two rows' indices and four palette codes -- its share of the
// two palettes.  At consumption the lane looks its four codes up in the dictionary and stores the doubles into the wavefront's
// own LDS area (2 x 128 doubles: [slice of the pair][slot][index]); the sixteen values of its two rows are then read from
// there.  Nobody but the wavefront touches the area: the order is program order (LDS serves a wavefront's accesses in order),
// kept for the compiler by wavefront-scope fences; no workgroup barrier in the loop.  The doubles that meet x are the
// dictionary's, in the same order: the same bits.  A slice that is not packed is served by its own mark, in the pair form (the
// lanes of its half) and in the lane-per-row form alike: its 16-bit codes are loaded where the slice is worked on (rare: the
// stage holds four dwords, not eight); a packed slice in the lane-per-row form: 8 B of stream per lane, its half of the area.
template <bool DOT, bool SR, bool NT, bool PAL>
__global__ __launch_bounds__(SP_BLOCK, SR ? SP_ONE_WGS_SR : SP_ONE_WGS) void spmv_one_kernel(
    const int2* __restrict__ p_desc, const unsigned long long* __restrict__ p_smode, const uint8_t* __restrict__ p_pairs,
    const double* __restrict__ p_svals, const uint16_t* __restrict__ p_c16, const int32_t* __restrict__ p_meta,
    const uint16_t* __restrict__ p_vcode, const uint2* __restrict__ p_pal, const uint8_t* __restrict__ p_palok,
    const double* __restrict__ p_dict, const double* __restrict__ p_x, double* __restrict__ p_y,
    const double* __restrict__ p_rvec, const int32_t* __restrict__ p_list, PipeArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double pp_lds[]; // the value dictionary
  __shared__ double red[SP_BLOCK / 64];
  __shared__ __attribute__((aligned(16))) double pal_area[PAL ? (SP_BLOCK / 64) * 256 : 2]; // per wavefront 2 x [8 slots][16]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const double* dict = pp_lds;

  // steps: a workgroup takes two groups of four slices at a time (list entries 2 t, 2 t + 1, or groups 2 t, 2 t + 1), wavefront
  // wv the slices 4 g + 2 (wv & 1), + 1 of group g = the (wv >> 1)-th of the two
  const int64_t ngroups = p_list ? a.nlist : ((int64_t)a.nslices + 3) / 4;
  const int64_t nitems = (ngroups + 1) / 2;
  const int xcd = blockIdx.x & 7;
  const int64_t lo = nitems * xcd / 8, hi = nitems * (xcd + 1) / 8;
  const int n_in_xcd = ((int)gridDim.x + 7 - xcd) >> 3;
  const int64_t first_item = lo + (blockIdx.x >> 3);
  const int n_steps = first_item < hi ? (int)((hi - first_item + n_in_xcd - 1) / n_in_xcd) : 0;

  // look-ahead registers, lane l <-> step regs_base + l: per slice chunk | width << 25 | class << 29 | exists << 31;
  // the first slice's index, bit 30: an affine pair, bits 28, 29: the first, the second slice is packed
  int r_ia = 0, r_ib = 0, r_s = 0;
  auto load_regs = [&](int base) {
    const int i = base + lane;
    const bool valid = i < n_steps;
    const int64_t t = first_item + (int64_t)(valid ? i : 0) * n_in_xcd;
    const int64_t gi = 2 * t + (wv >> 1);
    const bool have = valid && gi < ngroups;
    const int64_t g = (have && p_list) ? p_list[gi] : gi;
    const int64_t sa = 4 * g + 2 * (wv & 1);
    auto slice_info = [&](int64_t s64) -> int {
      if (!(have && s64 < a.nslices))
        return 0;
      const int2 d = p_desc[s64];
      const unsigned sm = (unsigned)p_smode[s64];
      const int nch = d.y & 0xffffff;
      return (nch ? d.x : 0) | ((nch ? (int)((unsigned)d.y >> 24) : 0) << 25) | ((nch ? (int)(sm & 3u) : 0) << 29) | (int)0x80000000;
    };
    r_ia = slice_info(sa);
    r_ib = slice_info(sa + 1);
    bool pr = have && sa + 1 < a.nslices && p_pairs[sa >> 1] != 0;
    const bool pka = PAL && have && sa < a.nslices && p_palok[sa] != 0;
    const bool pkb = PAL && have && sa + 1 < a.nslices && p_palok[sa + 1] != 0;
    r_s = have ? ((int)sa | (pr ? 0x40000000 : 0) | (pka ? 0x10000000 : 0) | (pkb ? 0x20000000 : 0)) : 0;
  };
  load_regs(0);
  if (a.stop_flag && *a.stop_flag)
    return;
  {
    // the dictionary into LDS: every thread's (at most eight) entries requested together, one round trip
    double t[SP_DICT_LDS_ENTRIES / SP_BLOCK];
#pragma unroll
    for (int i = 0; i < SP_DICT_LDS_ENTRIES / SP_BLOCK; ++i)
    {
      const int k = (int)threadIdx.x + i * SP_BLOCK;
      t[i] = k < a.dict_n ? p_dict[k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < SP_DICT_LDS_ENTRIES / SP_BLOCK; ++i)
    {
      const int k = (int)threadIdx.x + i * SP_BLOCK;
      if (k < a.dict_n)
        pp_lds[k] = t[i];
    }
  }
  __syncthreads();

  // descriptors: the codes, x, y (and r) -- offsets below 4 GB (the launcher sees to it)
  const int nb8 = a.nrows * 8;
  const __amdgpu_buffer_rsrc_t rs_vq = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p_vcode), 0, a.nslices * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_pq = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint2*>(p_pal), 0, PAL ? a.nslices * 512 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(p_x), 0, nb8, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(p_y, 0, nb8, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(SR ? p_rvec : p_x), 0, nb8, 0x00020000);
  const int lane8 = lane * 8, lane16 = lane * 16;
  const int aux = NT ? 2 : 0;

  struct Two
  {
    int ba[8];          // slot bases of the first slice (scalars; word 0 with the mode bits; a pair's second: 64 on)
    uint4v c0, c1;      // value codes: pair form, the lane's rows 2 l and 2 l + 1; else the lane's row of either slice
                        // (PAL: c0 alone -- pair form, the lane's 16 B of the packed blocks; else .xy, .zw its 8 B of either slice's)
  };
  double* const area = pal_area + (PAL ? wv * 256 : 0);
  // requested behind the gathers of the step before: bases (scalar loads), value codes
  auto prefetch = [&](Two& S, int ia, int ib, int sw) {
    const int ca = ia & 0x1ffffff, cb = ib & 0x1ffffff;
    const int32_t* __restrict__ ma = p_meta + (int64_t)ca * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      S.ba[e] = ma[e];
    if (PAL)
    {
      if (sw & 0x40000000)
      {
        const auto q = __builtin_amdgcn_raw_buffer_load_b128(rs_pq, ((lane < 32 ? ca : cb) << 9) + ((lane & 31) << 4), 0, aux);
        S.c0.x = q[0], S.c0.y = q[1], S.c0.z = q[2], S.c0.w = q[3];
      }
      else
      {
        // (an unpacked slice's block holds zeros, a missing slice reads chunk 0's: loaded, not used)
        const auto t0 = __builtin_amdgcn_raw_buffer_load_b64(rs_pq, (ca << 9) + lane8, 0, aux);
        const auto t1 = __builtin_amdgcn_raw_buffer_load_b64(rs_pq, (cb << 9) + lane8, 0, aux);
        S.c0.x = t0[0], S.c0.y = t0[1], S.c0.z = t1[0], S.c0.w = t1[1];
      }
      return;
    }
    int off0, off1;
    if (sw & 0x40000000)
    {
      // rows 2 l and 2 l + 1 of the 128: lanes 0..31 in the first chunk, 32..63 in the second, 32 contiguous bytes per lane
      off0 = ((lane < 32 ? ca : cb) << 10) + ((lane & 31) << 5);
      off1 = off0 + 16;
    }
    else
    {
      off0 = (ca << 10) + lane16;
      off1 = (cb << 10) + lane16;
    }
    const auto q0 = __builtin_amdgcn_raw_buffer_load_b128(rs_vq, off0, 0, aux);
    const auto q1 = __builtin_amdgcn_raw_buffer_load_b128(rs_vq, off1, 0, aux);
    S.c0.x = q0[0], S.c0.y = q0[1], S.c0.z = q0[2], S.c0.w = q0[3];
    S.c1.x = q1[0], S.c1.y = q1[1], S.c1.z = q1[2], S.c1.w = q1[3];
  };
  // a slice's column codes, where it has any (the lane-per-row form only; loaded when the slice is worked on: such slices are
  // the mesh's corners and edges on a regular mesh)
  auto load_codes = [&](int info) -> uint4v {
    const int c = info & 0x1ffffff, cls = (info >> 29) & 3;
    uint4v q = {0u, 0u, 0u, 0u};
    if (cls == SP_CLS_C16)
      q = vload<NT>(reinterpret_cast<const uint4v*>(p_c16 + (int64_t)c * 512) + lane);
    else if (cls != SP_CLS_NONE)
    {
      const char* cbase = cls == SP_CLS_C8T ? reinterpret_cast<const char*>(p_svals) + ((int64_t)c * 4096 + 3584)
                                            : reinterpret_cast<const char*>(p_c16) + (int64_t)c * 1024;
      const uint2v t = vload<NT>(reinterpret_cast<const uint2v*>(cbase) + lane);
      q.x = t.x, q.y = t.y;
    }
    return q;
  };

  RowSums Q;
  int regs_base = 0;
  auto step_scalars = [&](int i, int& ia, int& ib, int& sw) {
    if (i >= n_steps)
    {
      ia = ib = sw = 0;
      return;
    }
    if (i - regs_base >= 64)
    {
      regs_base = i;
      load_regs(regs_base);
      __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) here, on the rare path (see spmv_pipe_kernel)
    }
    ia = __builtin_amdgcn_readlane(r_ia, i - regs_base);
    ib = __builtin_amdgcn_readlane(r_ib, i - regs_base);
    sw = __builtin_amdgcn_readlane(r_s, i - regs_base);
  };

  // one slice in the lane-per-row form: W gathers, W dictionary look-ups, W products; `between`: what is requested behind the gathers
  // (PAL: vq.xy = the lane's 8 B of a packed slice, half = which half of the wavefront's area the slice's palettes take;
  // an unpacked slice's codes are loaded here)
  auto slice = [&](auto wtag, const int (&b)[8], uint4v vq, int info, int s, bool packed, int half, auto&& between) {
    constexpr int W = decltype(wtag)::value;
    const int w = (info >> 25) & 15, cls = (info >> 29) & 3;
    const uint4v cq = load_codes(info);
    if (PAL && !packed)
    {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(rs_vq, ((info & 0x1ffffff) << 10) + lane16, 0, aux);
      vq.x = q[0], vq.y = q[1], vq.z = q[2], vq.w = q[3];
    }
    unsigned cc[8];
    if (cls == SP_CLS_C16)
    {
      cc[0] = cq.x & 0xffffu, cc[1] = cq.x >> 16, cc[2] = cq.y & 0xffffu, cc[3] = cq.y >> 16;
      cc[4] = cq.z & 0xffffu, cc[5] = cq.z >> 16, cc[6] = cq.w & 0xffffu, cc[7] = cq.w >> 16;
    }
    else if (cls != SP_CLS_NONE)
    {
      cc[0] = cq.x & 0xffu, cc[1] = (cq.x >> 8) & 0xffu, cc[2] = (cq.x >> 16) & 0xffu, cc[3] = cq.x >> 24;
      cc[4] = cq.y & 0xffu, cc[5] = (cq.y >> 8) & 0xffu, cc[6] = (cq.y >> 16) & 0xffu, cc[7] = cq.y >> 24;
    }
    else
    {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        cc[e] = lane;
    }
    const unsigned vc[8] = {vq.x & 0xffffu, vq.x >> 16, vq.y & 0xffffu, vq.y >> 16, vq.z & 0xffffu, vq.z >> 16, vq.w & 0xffffu, vq.w >> 16};
    double xv[W > 0 ? W : 1], v[W > 0 ? W : 1];
#pragma unroll
    for (int e = 0; e < W; ++e)
    {
      const unsigned base = e == 0 ? (unsigned)(b[0] & 0x1fffffff) : (unsigned)b[e];
      // (a narrow slice, W = 8 > w: a slot beyond the width reads the column the packer left there, 0: a valid entry)
      xv[e] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(p_x) + ((base + ((W == 8 && e >= w) ? 0u : cc[e])) << 3));
    }
    double xr = 0.0, rr = 0.0;
    if (DOT)
    {
      const auto u = __builtin_amdgcn_raw_buffer_load_b64(rs_x, lane8, s << 9, 0);
      xr = __hiloint2double((int)u[1], (int)u[0]);
      if (SR)
      {
        const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs_r, lane8, s << 9, 0);
        rr = __hiloint2double((int)t[1], (int)t[0]);
      }
    }
    if (PAL && packed)
    {
      double* const ah = area + half * 128;
      dbl2 t;
      t.x = dict[vq.y & 0xffffu], t.y = dict[vq.y >> 16];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      *reinterpret_cast<dbl2*>(ah + 2 * lane) = t;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int e = 0; e < W; ++e)
        v[e] = ah[e * 16 + ((vq.x >> (4 * e)) & 15u)];
    }
    else
    {
#pragma unroll
      for (int e = 0; e < W; ++e)
        v[e] = dict[vc[e]];
    }
    between();
    double sum = 0.0;
#pragma unroll
    for (int e = 0; e < W; ++e)
      if (W < 8 || e < w)
        sum += v[e] * xv[e];
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uint2v, sum), rs_y, lane8, s << 9, 0);
    if (DOT && (s << 6) + lane < a.nrows) // (no row, no term: a lane without a row may hold 0 * inf)
      row_sums(Q, SR, a.nn_is_rr, sum, xr, rr);
  };
  auto slice_w = [&](const int (&b)[8], const uint4v vq, int info, int s, bool packed, int half, auto&& between) {
    if (info >= 0) // no such slice
    {
      between();
      return;
    }
    const int w = (info >> 25) & 15;
    if (w == 7)
      slice(std::integral_constant<int, 7>(), b, vq, info, s, packed, half, between);
    else
      slice(std::integral_constant<int, 8>(), b, vq, info, s, packed, half, between);
  };

  // one step: consume stage S (scalars ia, ib, sw), request the next step's stream into stage N
  auto body = [&](Two& S, int ia, int ib, int sw, Two& N, int ia_n, int ib_n, int sw_n) {
    const int sa = sw & 0x0fffffff;
    auto request_next = [&]() {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): the look-ups are back before scalar loads are in flight (they return out of order)
      prefetch(N, ia_n, ib_n, sw_n);
      __builtin_amdgcn_sched_barrier(0);
    };
    if (sw & 0x40000000)
    {
      // an affine pair: the lane's rows are 2 l and 2 l + 1 of the 128; slot e is the run of 128 doubles from ba[e]
      const int w = (ia >> 25) & 15;
      auto pair = [&](auto wtag, auto dtag, auto mtag) {
        constexpr int W = decltype(wtag)::value;
        // MIX (PAL only): one of the pair's slices, or both, are not packed -- the lanes of such a half load their rows' 16-bit
        // codes here and look the values up in the dictionary.  The pair keeps the pair form, so that a lane sums the same rows'
        // <p, A p> terms whether the stream is packed or not: solves agree bit for bit with ZZZ_SELLP_PAL=0.
        constexpr bool MIX = decltype(mtag)::value;
        // D >= 1: slot D is the DIAGONAL's (its run starts at the pair's first row) and slots D - 1, D, D + 1 start at
        // consecutive columns (c - 1, c, c + 1: the mesh line's own neighbours) -- the caller has checked both on the slots'
        // bases (scalars).  Two loads are saved per pair then: the middle run is the outer two's inner halves,
        // x[c + 2 l] = .y of slot D - 1, x[c + 2 l + 1] = .x of slot D + 1: not loaded; and it IS the rows' own x for
        // <x, A x>: no 16-B load of x at the rows themselves.  D = -1: every slot loaded, the rows' x too.  (Decided per slot
        // inside one body the same savings cost ~70 selects per pair: 13.4 M against 7.9 M vector instructions per product.)
        constexpr int D = decltype(dtag)::value;
        dbl2u xq[W];
#pragma unroll
        for (int e = 0; e < W; ++e)
        {
          if (e == D)
            continue;
          const unsigned base = e == 0 ? (unsigned)(S.ba[0] & 0x1fffffff) : ((W == 8 && e >= w) ? 0u : (unsigned)S.ba[e]);
          xq[e] = *reinterpret_cast<const dbl2u*>(reinterpret_cast<const char*>(p_x) + ((base << 3) + lane16));
        }
        if (D >= 1)
        {
          xq[D >= 1 ? D : 1].x = xq[D >= 1 ? D - 1 : 0].y;
          xq[D >= 1 ? D : 1].y = xq[D >= 1 ? D + 1 : 2].x;
        }
        double xr0 = 0.0, xr1 = 0.0, rr0 = 0.0, rr1 = 0.0;
        if (DOT)
        {
          if (D >= 1)
          {
            xr0 = xq[D >= 1 ? D : 1].x;
            xr1 = xq[D >= 1 ? D : 1].y;
          }
          else
          {
            const auto u = __builtin_amdgcn_raw_buffer_load_b128(rs_x, lane16, sa << 9, 0);
            xr0 = __hiloint2double((int)u[1], (int)u[0]);
            xr1 = __hiloint2double((int)u[3], (int)u[2]);
          }
          if (SR)
          {
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs_r, lane16, sa << 9, 0);
            rr0 = __hiloint2double((int)t[1], (int)t[0]);
            rr1 = __hiloint2double((int)t[3], (int)t[2]);
          }
        }
        // the stream of the next step goes out behind the gathers; the values are looked up as the products need them (the
        // codes stay packed until then: registers)
        const uint4v c0 = S.c0, c1 = S.c1;
        __builtin_amdgcn_sched_barrier(0);
        prefetch(N, ia_n, ib_n, sw_n);
        __builtin_amdgcn_sched_barrier(0);
        auto code = [](const uint4v& c, int e) -> unsigned {
          const unsigned wd = e < 2 ? c.x : (e < 4 ? c.y : (e < 6 ? c.z : c.w));
          return (e & 1) ? wd >> 16 : wd & 0xffffu;
        };
        double s0 = 0.0, s1 = 0.0;
        if (PAL)
        {
          // the lane's four palette entries into the wavefront's area (entries 4 l .. 4 l + 3 of the 256: lanes 32.. fill the
          // second slice's half), then the rows' values from the lane's half by their 4-bit indices
          dbl2 t0, t1;
          t0.x = dict[c0.y & 0xffffu], t0.y = dict[c0.y >> 16];
          t1.x = dict[c0.w & 0xffffu], t1.y = dict[c0.w >> 16];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          *reinterpret_cast<dbl2*>(area + 4 * lane) = t0;
          *reinterpret_cast<dbl2*>(area + 4 * lane + 2) = t1;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const double* const ah = area + (lane >> 5) * 128;
          // (an unpacked slice's block is zeros: its lanes have stored dictionary entry 0 and read it here, for nothing)
          uint4v u0 = {0u, 0u, 0u, 0u}, u1 = {0u, 0u, 0u, 0u};
          bool coded = false;
          if (MIX)
          {
            coded = ((lane < 32 ? sw & 0x10000000 : sw & 0x20000000)) == 0;
            if (coded)
            {
              const int off = (((lane < 32 ? ia : ib) & 0x1ffffff) << 10) + ((lane & 31) << 5);
              const auto q0 = __builtin_amdgcn_raw_buffer_load_b128(rs_vq, off, 0, aux);
              const auto q1 = __builtin_amdgcn_raw_buffer_load_b128(rs_vq, off + 16, 0, aux);
              u0.x = q0[0], u0.y = q0[1], u0.z = q0[2], u0.w = q0[3];
              u1.x = q1[0], u1.y = q1[1], u1.z = q1[2], u1.w = q1[3];
            }
          }
#pragma unroll
          for (int e = 0; e < W; ++e)
            if (W < 8 || e < w)
            {
              const double v0 = ah[e * 16 + ((c0.x >> (4 * e)) & 15u)], v1 = ah[e * 16 + ((c0.z >> (4 * e)) & 15u)];
              s0 += (MIX && coded ? dict[code(u0, e)] : v0) * xq[e].x;
              s1 += (MIX && coded ? dict[code(u1, e)] : v1) * xq[e].y;
            }
        }
        else
        {
#pragma unroll
          for (int e = 0; e < W; ++e)
            if (W < 8 || e < w) // (W = 8 also serves the narrow pairs: a slot beyond the width has read run 0, a valid one)
            {
              s0 += dict[code(c0, e)] * xq[e].x;
              s1 += dict[code(c1, e)] * xq[e].y;
            }
        }
        uint4v out;
        out.x = (unsigned)__double2loint(s0), out.y = (unsigned)__double2hiint(s0);
        out.z = (unsigned)__double2loint(s1), out.w = (unsigned)__double2hiint(s1);
        __builtin_amdgcn_raw_buffer_store_b128(out, rs_y, lane16, sa << 9, 0); // (rows beyond the last: the range check)
        if (DOT)
        {
          // row 2 l before row 2 l + 1.  row_sums' text, kept here by hand: through the helper the eight pair bodies' last sums
          // are merged behind their branches and the single-reduction form needs 100 registers instead of 89
          const int r0 = (sa << 6) + 2 * lane;
          if (r0 < a.nrows)
          {
            Q.dot += s0 * xr0;
            if (SR)
            {
              Q.dot_rx += rr0 * xr0;
              Q.dot_nn += a.nn_is_rr ? rr0 * rr0 : xr0 * xr0;
            }
          }
          if (r0 + 1 < a.nrows)
          {
            Q.dot += s1 * xr1;
            if (SR)
            {
              Q.dot_rx += rr1 * xr1;
              Q.dot_nn += a.nn_is_rr ? rr1 * rr1 : xr1 * xr1;
            }
          }
        }
      };
      // where the diagonal's slot sits between its two line neighbours (slot 3 of a lattice row's seven or eight entries, 4 where
      // an eighth comes first): the scalar test on the bases picks the body
      const unsigned rb = (unsigned)sa << 6;
      auto tri = [&](int d) {
        const unsigned bl = d - 1 == 0 ? (unsigned)(S.ba[0] & 0x1fffffff) : (unsigned)S.ba[d - 1];
        return d + 1 < w && (unsigned)S.ba[d] == rb && bl + 1u == rb && (unsigned)S.ba[d + 1] == rb + 1u;
      };
      const int dsel = tri(3) ? 3 : (tri(4) ? 4 : -1);
      constexpr std::false_type all_packed;
      constexpr std::integral_constant<bool, PAL> not_all_packed; // (never taken without PAL: the body of all_packed again)
      if (PAL && (sw & 0x30000000) != 0x30000000) // (rare: the general body, every slot loaded)
      {
        if (w == 7)
          pair(std::integral_constant<int, 7>(), std::integral_constant<int, -1>(), not_all_packed);
        else
          pair(std::integral_constant<int, 8>(), std::integral_constant<int, -1>(), not_all_packed);
      }
      else if (w == 7)
      {
        if (dsel == 3)
          pair(std::integral_constant<int, 7>(), std::integral_constant<int, 3>(), all_packed);
        else if (dsel == 4)
          pair(std::integral_constant<int, 7>(), std::integral_constant<int, 4>(), all_packed);
        else
          pair(std::integral_constant<int, 7>(), std::integral_constant<int, -1>(), all_packed);
      }
      else
      {
        if (dsel == 3)
          pair(std::integral_constant<int, 8>(), std::integral_constant<int, 3>(), all_packed);
        else if (dsel == 4)
          pair(std::integral_constant<int, 8>(), std::integral_constant<int, 4>(), all_packed);
        else
          pair(std::integral_constant<int, 8>(), std::integral_constant<int, -1>(), all_packed);
      }
    }
    else
    {
      // the two slices one after the other, a lane per row; the next step's stream goes out behind the first one's gathers
      uint4v qb = S.c1;
      if (PAL)
        qb.x = S.c0.z, qb.y = S.c0.w; // (before request_next: the stage it fills may be read no later than that)
      slice_w(S.ba, S.c0, ia, sa, (sw & 0x10000000) != 0, 0, request_next);
      int bb[8]; // (the second slice's bases: loaded here, this path is the rare one)
      const int32_t* __restrict__ mb = p_meta + (int64_t)(ib & 0x1ffffff) * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        bb[e] = mb[e];
      slice_w(bb, qb, ib, sa + 1, (sw & 0x20000000) != 0, 1, []() {});
    }
  };

  Two A, B;
  int ia_a, ib_a, sw_a, ia_b, ib_b, sw_b;
  step_scalars(0, ia_a, ib_a, sw_a);
  prefetch(A, ia_a, ib_a, sw_a);
  for (int i = 0; i < n_steps;)
  {
    step_scalars(i + 1, ia_b, ib_b, sw_b);
    body(A, ia_a, ib_a, sw_a, B, ia_b, ib_b, sw_b);
    if (++i >= n_steps)
      break;
    step_scalars(i + 1, ia_a, ib_a, sw_a);
    body(B, ia_b, ib_b, sw_b, A, ia_a, ib_a, sw_a);
    ++i;
  }

  if (DOT)
    row_sums_store(Q, SR, false, a.partials, a.pstride, red);
}

// the pairs of a freshly packed stream of one-chunk slices (called by the stream's first use, behind the dictionary build)
int sellp_pairs_build(zzz_ctx* ctx)
{
  const int64_t npairs = (ctx->nslices + 1) / 2;
  ZZZ_HIP(ctx, ctx->sp_pairs.alloc((size_t)npairs + 1));
  hipLaunchKernelGGL(k_sp_pairs, dim3((unsigned)std::min<int64_t>((npairs + 255) / 256, 4096)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<const int2*>(ctx->sp_desc.p), ctx->sp_smode.p, ctx->sp_meta.p, ctx->nslices, ctx->sp_pairs.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// Does the kernel serve this context's stream, and with how many workgroups per CU?  0: the generic kernel.  (What a launch
// adds: no Chebyshev epilogue.)
int sellp_pipe_wgs(const zzz_ctx* ctx, bool sr)
{
  if (!ctx->knob.sellp_pipe || !ctx->values.sp_pipe_ok || ctx->sp_sorted || ctx->values.sp_chunks <= 0)
    return 0;
  if (!(ctx->values.sp_dict_on && ctx->sp_dict_n <= SP_DICT_LDS_ENTRIES && !ctx->values.sp_sd_on))
    return 0;
  if (!(ctx->values.sp_one_chunk && ctx->values.sp_pairs_ok && ctx->bs == 1 && ctx->values.sp_win_max == 0 && ctx->nslices < (1 << 21)))
    return 0;
  return sr ? SP_ONE_WGS_SR : SP_ONE_WGS;
}

// [mode][load]; a product with a Chebyshev term takes the generic kernel
using OneKernel = decltype(&spmv_one_kernel<false, false, false, false>);
template <bool PAL>
constexpr std::array<std::array<OneKernel, 2>, PM_PLAIN + 1> one_variants()
{
  return {{{spmv_one_kernel<true, true, true, PAL>, spmv_one_kernel<true, true, false, PAL>},
           {spmv_one_kernel<true, false, true, PAL>, spmv_one_kernel<true, false, false, PAL>},
           {spmv_one_kernel<false, false, true, PAL>, spmv_one_kernel<false, false, false, PAL>}}};
}
static const std::array<std::array<OneKernel, 2>, PM_PLAIN + 1> one_kernels[2] = {one_variants<false>(), one_variants<true>()}; // [packed form]

bool launch_sellp_pipe(zzz_ctx* ctx, int grid, const ProductCall& c)
{
  if (c.epi || !sellp_pipe_wgs(ctx, c.mode == PM_DOT_SR))
    return false;
  PipeArgs a;
  a.dict_n = ctx->sp_dict_n;
  a.nrows = (int)ctx->nrows;
  a.nslices = (int)ctx->nslices;
  product_args_tail(a, c);
  const size_t lds = (size_t)((ctx->sp_dict_n + 1) & ~1) * sizeof(double);
  hipLaunchKernelGGL(one_kernels[ctx->values.sp_pal_on ? 1 : 0][c.mode][c.load], dim3(grid), dim3(SP_BLOCK), lds, ctx->stream,
                     reinterpret_cast<const int2*>(ctx->sp_desc.p), ctx->sp_smode.p, ctx->sp_pairs.p, ctx->sp_vals.p, ctx->sp_codes16.p,
                     ctx->sp_meta.p, ctx->sp_vcode.p, ctx->sp_pal.p, ctx->sp_palok.p, ctx->sp_dset.dict.p, c.x, c.y, c.rvec, c.list, a);
  return true;
}
ZZZ_PRELOAD_TU(sellp_pipe)
} // namespace zzz
