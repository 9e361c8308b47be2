// Host-side helpers of the set-up code: rocPRIM's device scans, sorts and selects with their scratch, the grid of a
// grid-stride kernel, a scalar read back from the device.  Not part of the ABI.
#pragma once
#include <cstring> // (rocPRIM's texture_cache_iterator.hpp calls memset without including it)

#include <rocprim/rocprim.hpp>

#include "zzz_internal.h"

namespace zzz
{
// a grid of at most `cap` workgroups for `items` items at `per` each
inline int grid_cap(int64_t items, int per, int cap)
{
  int64_t g = (items + per - 1) / per;
  if (g > cap)
    g = cap;
  if (g < 1)
    g = 1;
  return (int)g;
}

// `count` values from the device, waited for: the total behind a scan, a flag a kernel has left
template <typename T>
inline hipError_t dev_fetch(zzz_ctx* ctx, const T* device, T* host, size_t count = 1)
{
  const hipError_t e = hipMemcpyAsync(host, device, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

// ---- scratch of a device primitive ---------------------------------------------------------------------------------
// A primitive is a callable  hipError_t(void* tmp, size_t& bytes)  around ONE rocPRIM call: with_scratch asks it for its
// size (tmp == null: nothing is launched), obtains that much and runs it.  Where the scratch lives is the caller's choice:
//   with_scratch(ctx, call)        the context's shared scratch.  It only grows, and a buffer that is too small is RETIRED
//                                  (DevBuf::grow_keep), never freed: hipFree waits for every kernel on the device, and on a
//                                  GPU shared by two ranks the other rank's kernel may be polling its mailbox for this one.
//                                  Every set-up step that runs per assembly or on a live context belongs here.
//   with_scratch(ctx, tmp, call)   a buffer of the caller's, grown within its lifetime and freed with it: the large
//                                  one-off sorts, which a context should not keep for life.  The caller waits for the
//                                  stream before `tmp` goes out of scope.
inline hipError_t scratch_reserve(zzz_ctx* ctx, size_t bytes) { return ctx->scr_tmp.grow_keep(bytes, ctx->retired); }

template <typename F>
inline hipError_t scratch_bytes(F call, size_t* bytes)
{
  *bytes = 0;
  return call(nullptr, *bytes);
}

template <typename F>
inline int with_scratch(zzz_ctx* ctx, F call)
{
  size_t bytes = 0;
  ZZZ_HIP(ctx, call(nullptr, bytes));
  ZZZ_HIP(ctx, scratch_reserve(ctx, bytes));
  ZZZ_HIP(ctx, call((void*)ctx->scr_tmp.p, bytes));
  return ZZZ_OK;
}

template <typename F>
inline int with_scratch(zzz_ctx* ctx, DevBuf<unsigned char>& tmp, F call)
{
  size_t bytes = 0;
  ZZZ_HIP(ctx, call(nullptr, bytes));
  ZZZ_HIP(ctx, tmp.reserve(bytes));
  ZZZ_HIP(ctx, call((void*)tmp.p, bytes));
  return ZZZ_OK;
}

// ---- the two primitives most sites use, as callables for with_scratch ------------------------------------------------
// out[i] = in[0] + ... + in[i - 1], summed in T, for i < n (`in`: a pointer or an iterator)
template <typename In, typename T>
inline auto scan_excl(In in, T* out, size_t n, hipStream_t s)
{
  return [=](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), s); };
}

// stable sort of n (key, value) pairs by bits [begin_bit, end_bit) of the keys
template <typename K, typename V>
inline auto sort_pairs(K* kin, K* kout, V* vin, V* vout, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s)
{
  return [=](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, s);
  };
}

// ... and of n keys alone
template <typename K>
inline auto sort_keys(K* kin, K* kout, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s)
{
  return [=](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys(tmp, bytes, kin, kout, n, begin_bit, end_bit, s); };
}
} // namespace zzz
