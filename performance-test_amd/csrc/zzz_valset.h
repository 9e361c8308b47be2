// Sets of distinct double values numbered into 16-bit codes: the stream's value dictionary (zzz_sellp_dict.hip), Jacobi's
// inverse diagonal as codes (zzz_cg.hip) and the block-row form's value dictionary (form 2, zzz_sellp_blk.hip).  An
// open-addressing set of 2^BITS 64-bit patterns in global memory, ~0ull the empty marker (a NaN no assembled value has; met
// all the same, the set declines).  The callers' kernels walk their values into valset_insert / valset_insert_wave;
// k_valset_number gives them codes from FIRST on (FIRST = 1: code 0 stands for +0.0, which the callers never insert);
// valset_find turns a value back into its code.  The LDS sets of k_sp_sd_build and k_bw_values take only the hash.
// Counters (ValSet::info): [0] values inserted, [1] nonzero when the set declines, [2] entries numbered (code 0 included).
// A set declines when more than `limit` values go in (+0.0 not counted where code 0 stands for it):
//   stream dictionary   2 046 (the LDS copy holds 2 048 entries); 65 534 with ZZZ_SELLP_DICT=2
//   Jacobi codes        2 048 (+0.0 would be counted)
//   block-row values    2 046
// Included by zzz_internal.h, after DevBuf.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

namespace zzz
{
constexpr unsigned long long VALSET_EMPTY = ~0ull;

template <int BITS>
__device__ inline unsigned valset_hash(uint64_t b)
{
  b ^= b >> 29;
  b *= 0x9E3779B97F4A7C15ull;
  return (unsigned)(b >> (64 - BITS));
}

// The flag and the slots are read past the L1 cache: a slot cached as empty before another CU's insertion would send every
// later occurrence of that value to the atomic (3.4 ms at 1.25 M rows instead of 0.05).
__device__ inline bool valset_declined(int* info) { return __hip_atomic_load(&info[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }

// one lane's value into the set
template <int BITS>
__device__ inline void valset_insert(unsigned long long* table, int* info, int limit, unsigned long long b)
{
  if (b == VALSET_EMPTY)
  {
    info[1] = 1;
    return;
  }
  unsigned h = valset_hash<BITS>(b);
  for (int probe = 0; probe < (1 << BITS); ++probe)
  {
    const unsigned long long cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == b)
      break;
    if (cur == VALSET_EMPTY)
    {
      const unsigned long long old = atomicCAS(&table[h], VALSET_EMPTY, b);
      if (old == VALSET_EMPTY)
      {
        if (atomicAdd(&info[0], 1) >= limit)
          info[1] = 1;
        break;
      }
      if (old == b)
        break;
    }
    h = (h + 1) & ((1u << BITS) - 1);
    if (valset_declined(info))
      break; // (the table may be filling up: stop looking)
  }
}

// The values of the lanes with `need` into the set, one lane per distinct value of the wavefront (the lanes of a wavefront
// mostly hold the same few values).  Every lane of the wavefront calls it; false: the set has declined, stop walking.
template <int BITS>
__device__ inline bool valset_insert_wave(unsigned long long* table, int* info, int limit, unsigned long long b, bool need)
{
  for (unsigned long long todo = __ballot(need); todo; todo = __ballot(need))
  {
    if (valset_declined(info))
      return false; // (the waves in flight when the limit is met would fill the table up otherwise)
    const int src = __ffsll((long long)todo) - 1;
    const unsigned long long bb = ((unsigned long long)(unsigned)__shfl((int)(b >> 32), src) << 32) | (unsigned)__shfl((int)(unsigned)b, src);
    if ((int)(threadIdx.x & 63) == src)
      valset_insert<BITS>(table, info, limit, bb);
    need = need && b != bb;
  }
  return true;
}

// the code of a value that is in the set
template <int BITS>
__device__ inline int valset_find(const unsigned long long* table, const int32_t* slot_code, unsigned long long b)
{
  unsigned h = valset_hash<BITS>(b);
  while (table[h] != b)
    h = (h + 1) & ((1u << BITS) - 1);
  return slot_code[h];
}

// Numbers the occupied slots of a table of 2^BITS (slots != empty) from FIRST on, in one workgroup of 1 024 threads: thread t
// takes slots t, t + 1 024, t + 2 048, ... (coalesced reads) and gives the occupied ones consecutive codes, threads in order.
// emit(slot, code, pattern) per occupied slot.  Returns the code after the last, FIRST + the occupied slots, in every thread.
template <int BITS, int FIRST, class Emit>
__device__ inline int valset_number(const unsigned long long* table, unsigned long long empty, Emit emit)
{
  __shared__ int wsum[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int mine = 0;
  for (int k = threadIdx.x; k < (1 << BITS); k += 1024)
    mine += table[k] != empty ? 1 : 0;
  int incl = mine; // inclusive scan of `mine` over the wavefront
  for (int d = 1; d < 64; d <<= 1)
  {
    const int t = __shfl_up(incl, d);
    if (lane >= d)
      incl += t;
  }
  if (lane == 63)
    wsum[wv] = incl;
  __syncthreads();
  int code = FIRST + incl - mine, total = FIRST;
  for (int q = 0; q < 16; ++q)
  {
    code += q < wv ? wsum[q] : 0;
    total += wsum[q];
  }
  for (int k = threadIdx.x; k < (1 << BITS); k += 1024)
  {
    const unsigned long long b = table[k];
    if (b != empty)
      emit(k, code++, b);
  }
  return total;
}

// slot -> code, code -> value (dict: `cap` entries); nothing when the set has declined
template <int BITS, int FIRST>
__global__ __launch_bounds__(1024) void k_valset_number(const unsigned long long* __restrict__ table, int32_t* __restrict__ slot_code,
                                                        double* __restrict__ dict, int* __restrict__ info, int cap)
{
  if (info[1])
    return;
  const int n = valset_number<BITS, FIRST>(table, VALSET_EMPTY, [&](int k, int code, unsigned long long b) {
    slot_code[k] = code;
    if (code < cap)
      dict[code] = __longlong_as_double((long long)b);
  });
  if (threadIdx.x == 0)
  {
    if (FIRST)
      dict[0] = 0.0;
    info[2] = n;
  }
}

// The buffers of one set on a context.  Grown only (DevBuf::grow_keep: they may be asked for while another context's kernel
// waits on this GPU); their sizes are fixed by BITS and the dictionary's capacity, so they are allocated once.
// begin (buffers, counters cleared, table emptied), the caller's insert pass, number, the caller's encode pass, finish: the
// encode pass goes between number and finish so that a build synchronises once.
template <int BITS, int FIRST>
struct ValSet
{
  static constexpr int bits = BITS;
  DevBuf<unsigned long long> table; // the set (build only)
  DevBuf<int32_t> slot;             // table slot -> code (build only)
  DevBuf<double> dict;              // code -> value, `cap` entries
  DevBuf<int32_t> info;             // counters (above)
  int cap = 0;

  hipError_t begin(int dict_cap, hipStream_t s, std::vector<void*>& retired)
  {
    cap = dict_cap;
    hipError_t e = table.grow_keep((size_t)1 << BITS, retired);
    if (e == hipSuccess)
      e = slot.grow_keep((size_t)1 << BITS, retired);
    if (e == hipSuccess)
      e = dict.grow_keep((size_t)cap, retired);
    if (e == hipSuccess)
      e = info.grow_keep(4, retired);
    if (e == hipSuccess)
      e = hipMemsetAsync(info.p, 0, 4 * sizeof(int32_t), s);
    if (e == hipSuccess)
      e = hipMemsetAsync(table.p, 0xff, sizeof(unsigned long long) << BITS, s);
    return e;
  }
  void number(hipStream_t s)
  {
    hipLaunchKernelGGL((k_valset_number<BITS, FIRST>), dim3(1), dim3(1024), 0, s, table.p, slot.p, dict.p, info.p, cap);
  }
  // synchronises the stream; entries = the dictionary's entries, 0 when the set declined
  hipError_t finish(hipStream_t s, int& entries)
  {
    entries = 0;
    int32_t h[4] = {0, 1, 0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
      e = hipMemcpyAsync(h, info.p, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
      e = hipStreamSynchronize(s);
    if (e == hipSuccess && !h[1] && h[2] > 0 && h[2] <= cap)
      entries = h[2];
    return e;
  }
};
} // namespace zzz
