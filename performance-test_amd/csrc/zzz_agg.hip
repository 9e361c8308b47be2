// ZZZ_PC_AGG: unsmoothed (plain) aggregation multigrid from the assembled matrix alone (PETSc's -pc_type gamg
// -pc_gamg_agg_nsmooths 0; the reference's README.md:59-146 recommends an algebraic multigrid preconditioner).  This file
// holds what is algebraic: the aggregation, the Galerkin coarse matrix and the two transfer kernels.  Levels, smoother,
// V-cycle, dense coarsest solve, caching and profiling are zzz_mg.hip's.
//
// The rule, per level (tests/_agg_ref.py restates it aggregate for aggregate):
//   graph      nodes: the block dofs with at least one unconstrained component; i ~ j when any scalar entry of their coupling
//              is nonzero.  A node whose components are all constrained stays out (zero rows of P); a constrained component
//              of a mixed node has a zero row of P too.  Coarse levels have no constrained dofs.
//   priority   of node i (its index in the CALLER's numbering on level 0, its index on a coarse level), in 64-bit unsigned
//              arithmetic:  x = i + 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
//              x *= 0x94D049BB133111EB;  x ^= x >> 31;  priority = ((x >> 33) << 32) | i  -- the index is part of it: no ties.
//   roots      a distance-2 maximal independent set in synchronous rounds: an undecided node becomes a root when its
//              priority exceeds that of every undecided node within distance 2 (paths run through graph nodes of any
//              state); every undecided node within distance 2 of a root then goes out.  Until nobody is undecided.
//   numbers    aggregates are numbered by ascending root index.
//   joins      two synchronous rounds: an unaggregated node joins the aggregate of its adjacent aggregated neighbour with
//              the largest aggregate number.
//   the rest   becomes singleton aggregates in index order, numbered behind the roots'.
// Nothing depends on thread scheduling: every round reads the state the previous kernel left and writes its own node only;
// the only atomics are an integer count and an integer maximum.
//
// P is 1 from each unconstrained scalar dof (i, c) to dof (aggregate(i), c): piecewise constant, one coarse dof per
// component, never stored -- the aggregate map and its inverse (members by ascending index) are the transfer.
// A_c = P^T A P: coarse entry (I, J) is the sum of the fine entries a_ij with i in I, j in J, summed in ascending fine
// (row, column) order of the caller's numbering: the entries' coarse keys go through a STABLE radix sort (rocPRIM), one
// thread then sums each run front to back -- two set-ups give the same bits, and a refresh is that sum alone.
//
// The aggregation reads its graph through AggGraph: a context's matrix with its block size (1 or 3), or -- for the coarse levels
// of ZZZ_PC_SAGG_RBM, whose nodes are blocks of six rows of a scalar matrix -- node rows written out by the caller
// (agg_aggregate_graph).
#include "zzz_cg.h"

#include "zzz_prim.h"

#include <algorithm>
#include <vector>

namespace zzz
{
constexpr int AGG_UNDECIDED = 0, AGG_ROOT = 1, AGG_OUT = 2, AGG_EXCLUDED = 3;
constexpr unsigned long long AGG_NOKEY = ~0ull;

struct AggLevel
{
  int bs = 1;
  int64_t nf = 0;   // fine block dofs
  int64_t nagg = 0; // aggregates
  int rounds = 0;   // rounds the independent set took
  DevBuf<int32_t> agg;       // [nf] aggregate of a fine block dof, -1: none (all components constrained)
  DevBuf<int32_t> moff, mem; // the map inverted: members of aggregate a are mem[moff[a] .. moff[a + 1]), ascending index
  // the Galerkin sum: fine entry src[t] belongs to coarse entry e for seg[e] <= t < seg[e + 1]
  int64_t nfine = 0, nnzc = 0;
  DevBuf<int32_t> src, seg;
};

__device__ inline long long agg_priority(long long idx)
{
  unsigned long long x = (unsigned long long)idx + 0x9E3779B97F4A7C15ull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (long long)(((x >> 33) << 32) | (unsigned long long)(unsigned)idx);
}

#define AGG_FOR(i, n) for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < (n); i += (int64_t)gridDim.x * VB)

// state and priority of every block dof; perm: internal -> caller index (null: the same)
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_init(int64_t n, const uint8_t* __restrict__ bc, const int32_t* __restrict__ perm,
                                                 int32_t* __restrict__ state, long long* __restrict__ key)
{
  AGG_FOR(i, n)
  {
    bool free_ = false;
#pragma unroll
    for (int c = 0; c < BS; ++c)
      free_ |= bc[i * BS + c] == 0;
    state[i] = free_ ? AGG_UNDECIDED : AGG_EXCLUDED;
    key[i] = agg_priority(perm ? perm[i] : i);
  }
}

// m1[i] = the largest priority among the undecided nodes of {i} and its neighbours (-1: none; a node out of the graph: -1)
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_max1(int64_t n, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                 const double* __restrict__ vals, const int32_t* __restrict__ state,
                                                 const long long* __restrict__ key, long long* __restrict__ m1)
{
  AGG_FOR(i, n)
  {
    const int si = state[i];
    long long m = si == AGG_UNDECIDED ? key[i] : -1;
    for (rp_t k = rowptr[i * BS]; k < rowptr[i * BS + BS]; ++k)
    {
      const int32_t j = cols[k] / BS;
      const double v = vals[k];
      const int sj = state[j];
      const long long kj = key[j];
      const long long cand = (v != 0.0 && sj == AGG_UNDECIDED) ? kj : -1;
      m = cand > m ? cand : m;
    }
    m1[i] = si == AGG_EXCLUDED ? -1 : m;
  }
}

// the maximum of the neighbours' maxima is the maximum within distance 2: an undecided node that holds it is a root
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_max2(int64_t n, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                 const double* __restrict__ vals, const long long* __restrict__ key,
                                                 const long long* __restrict__ m1, int32_t* __restrict__ state)
{
  AGG_FOR(i, n)
  {
    long long m = m1[i];
    for (rp_t k = rowptr[i * BS]; k < rowptr[i * BS + BS]; ++k)
    {
      const int32_t j = cols[k] / BS;
      const double v = vals[k];
      const long long mj = m1[j];
      const long long cand = v != 0.0 ? mj : -1;
      m = cand > m ? cand : m;
    }
    if (state[i] == AGG_UNDECIDED && m == key[i])
      state[i] = AGG_ROOT;
  }
}

// near[i] = a root in {i} and its neighbours
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_near1(int64_t n, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                  const double* __restrict__ vals, const int32_t* __restrict__ state,
                                                  uint8_t* __restrict__ near)
{
  AGG_FOR(i, n)
  {
    const int si = state[i];
    bool r = si == AGG_ROOT;
    for (rp_t k = rowptr[i * BS]; k < rowptr[i * BS + BS]; ++k)
    {
      const int32_t j = cols[k] / BS;
      const double v = vals[k];
      const int sj = state[j];
      r |= v != 0.0 && sj == AGG_ROOT;
    }
    near[i] = (r && si != AGG_EXCLUDED) ? 1 : 0;
  }
}

// an undecided node with a root within distance 2 goes out; the others are counted (an integer sum: any order)
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_near2(int64_t n, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                  const double* __restrict__ vals, const uint8_t* __restrict__ near,
                                                  int32_t* __restrict__ state, int32_t* __restrict__ undecided)
{
  AGG_FOR(i, n)
  {
    bool r = near[i] != 0;
    for (rp_t k = rowptr[i * BS]; k < rowptr[i * BS + BS]; ++k)
    {
      const int32_t j = cols[k] / BS;
      const double v = vals[k];
      const uint8_t nj = near[j];
      r |= v != 0.0 && nj != 0;
    }
    if (state[i] == AGG_UNDECIDED)
    {
      if (r)
        state[i] = AGG_OUT;
      else
        atomicAdd(undecided, 1);
    }
  }
}

// flags in the caller's order: what = 0 the roots, 1 the graph nodes without an aggregate
__global__ __launch_bounds__(VB) void k_agg_flags(int64_t n, int what, const int32_t* __restrict__ perm,
                                                  const int32_t* __restrict__ state, const int32_t* __restrict__ agg,
                                                  int32_t* __restrict__ flag)
{
  AGG_FOR(i, n)
  {
    const int64_t p = perm ? perm[i] : i;
    const int s = state[i];
    const int32_t a = agg[i];
    flag[p] = what == 0 ? (s == AGG_ROOT ? 1 : 0) : ((s != AGG_EXCLUDED && a < 0) ? 1 : 0);
    if (i == 0)
      flag[n] = 0;
  }
}
// ... and the numbers from their exclusive scan (flagged nodes only; the others keep what they have, the roots' pass: -1)
__global__ __launch_bounds__(VB) void k_agg_number(int64_t n, int what, int32_t base, const int32_t* __restrict__ perm,
                                                   const int32_t* __restrict__ flag, const int32_t* __restrict__ scan,
                                                   int32_t* __restrict__ agg)
{
  AGG_FOR(i, n)
  {
    const int64_t p = perm ? perm[i] : i;
    const int32_t f = flag[p], s = scan[p], a = agg[i];
    agg[i] = f ? base + s : (what == 0 ? -1 : a);
  }
}

// one joining round: in -> out
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_join(int64_t n, const rp_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                 const double* __restrict__ vals, const int32_t* __restrict__ state,
                                                 const int32_t* __restrict__ in, int32_t* __restrict__ out)
{
  AGG_FOR(i, n)
  {
    const int32_t a = in[i];
    int32_t best = -1;
    for (rp_t k = rowptr[i * BS]; k < rowptr[i * BS + BS]; ++k)
    {
      const int32_t j = cols[k] / BS;
      const double v = vals[k];
      const int32_t aj = in[j];
      const int32_t cand = v != 0.0 ? aj : -1;
      best = cand > best ? cand : best;
    }
    out[i] = (a < 0 && state[i] != AGG_EXCLUDED) ? best : a;
  }
}

// sort input of the inverted map, in the caller's order: key = aggregate (none: behind all), value = the node
__global__ __launch_bounds__(VB) void k_agg_member_keys(int64_t n, const int32_t* __restrict__ perm, const int32_t* __restrict__ agg,
                                                        uint32_t* __restrict__ key, int32_t* __restrict__ val)
{
  AGG_FOR(i, n)
  {
    const int64_t p = perm ? perm[i] : i;
    const int32_t a = agg[i];
    key[p] = a < 0 ? 0x7fffffffu : (uint32_t)a;
    val[p] = (int32_t)i;
  }
}

// off[a] = first position of key a in the ascending keys (a = 0 .. nseg; keys >= nseg are a tail that belongs to nobody)
template <typename K, typename O>
__global__ __launch_bounds__(VB) void k_agg_offsets(const K* __restrict__ keys, int64_t n, int64_t nseg, O* __restrict__ off)
{
  AGG_FOR(t, n + 1)
  {
    const int64_t a = (int64_t)keys[t > 0 ? t - 1 : 0], b = (int64_t)keys[t < n ? t : n - 1];
    const int64_t lo = t == 0 ? -1 : (a < nseg ? a : nseg);
    const int64_t hi = t == n ? nseg : (b < nseg ? b : nseg);
    for (int64_t s = lo + 1; s <= hi; ++s)
      off[s] = (O)t;
  }
}

// the scalar row of every fine entry
__global__ __launch_bounds__(VB) void k_agg_rowidx(int64_t nrows, const rp_t* __restrict__ rowptr, int32_t* __restrict__ rowidx)
{
  AGG_FOR(r, nrows)
    for (rp_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
      rowidx[k] = (int32_t)r;
}

// level 0 in an internal order: the entries' (row, column) in the caller's numbering, to be sorted first
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_caller_keys(int64_t nnz, const int32_t* __restrict__ rowidx, const int32_t* __restrict__ cols,
                                                        const int32_t* __restrict__ perm, unsigned long long* __restrict__ key,
                                                        int32_t* __restrict__ val)
{
  AGG_FOR(k, nnz)
  {
    const int32_t r = rowidx[k], c = cols[k];
    const unsigned long long R = (unsigned long long)perm[r / BS] * BS + (unsigned)(r % BS);
    const unsigned long long Cc = (unsigned long long)perm[c / BS] * BS + (unsigned)(c % BS);
    key[k] = (R << 32) | Cc;
    val[k] = (int32_t)k;
  }
}

// the coarse (row, column) of fine entry src[t] (src null: t), AGG_NOKEY where P has a zero row at either end
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_coarse_keys(int64_t nnz, const int32_t* __restrict__ src, const int32_t* __restrict__ rowidx,
                                                        const int32_t* __restrict__ cols, const uint8_t* __restrict__ bc,
                                                        const int32_t* __restrict__ agg, unsigned long long* __restrict__ key,
                                                        int32_t* __restrict__ val)
{
  AGG_FOR(t, nnz)
  {
    const int32_t k = src ? src[t] : (int32_t)t;
    const int32_t r = rowidx[k], c = cols[k];
    const int32_t I = agg[r / BS], J = agg[c / BS];
    const bool ok = I >= 0 && J >= 0 && bc[r] == 0 && bc[c] == 0;
    const unsigned long long R = (unsigned long long)(I >= 0 ? I : 0) * BS + (unsigned)(r % BS);
    const unsigned long long Cc = (unsigned long long)(J >= 0 ? J : 0) * BS + (unsigned)(c % BS);
    key[t] = ok ? ((R << 32) | Cc) : AGG_NOKEY;
    val[t] = k;
  }
}

// head[t] = sorted entry t opens a coarse entry
__global__ __launch_bounds__(VB) void k_agg_heads(int64_t nnz, const unsigned long long* __restrict__ key, int32_t* __restrict__ head)
{
  AGG_FOR(t, nnz)
  {
    const unsigned long long a = key[t > 0 ? t - 1 : 0], b = key[t];
    head[t] = (b != AGG_NOKEY && (t == 0 || a != b)) ? 1 : 0;
    if (t == 0)
      head[nnz] = 0;
  }
}

// coarse entry e = pos[t] of every head t: where its run starts, its column, its row; the end of the last run
__global__ __launch_bounds__(VB) void k_agg_entries(int64_t nnz, int64_t nnzc, const unsigned long long* __restrict__ key,
                                                    const int32_t* __restrict__ head, const int32_t* __restrict__ pos,
                                                    int32_t* __restrict__ seg, int32_t* __restrict__ ccols, int32_t* __restrict__ crow)
{
  AGG_FOR(t, nnz)
  {
    const unsigned long long b = key[t], nx = key[t + 1 < nnz ? t + 1 : t];
    const int32_t h = head[t], e = pos[t];
    if (h)
    {
      seg[e] = (int32_t)t;
      ccols[e] = (int32_t)(b & 0xffffffffull);
      crow[e] = (int32_t)(b >> 32);
    }
    if (b != AGG_NOKEY && (t + 1 == nnz || nx == AGG_NOKEY))
      seg[nnzc] = (int32_t)(t + 1);
  }
}

// the Galerkin sum: one thread per coarse entry, its run front to back
__global__ __launch_bounds__(VB) void k_agg_values(int64_t nnzc, const int32_t* __restrict__ seg, const int32_t* __restrict__ src,
                                                   const double* __restrict__ fine, double* __restrict__ coarse)
{
  AGG_FOR(e, nnzc)
  {
    double s = 0.0;
    for (int32_t t = seg[e]; t < seg[e + 1]; ++t)
      s += fine[src[t]];
    coarse[e] = s;
  }
}

// out[0] = the longest coarse row (an integer maximum), out[1] = the empty ones (an integer sum)
__global__ __launch_bounds__(VB) void k_agg_rowstats(int64_t nrows, const rp_t* __restrict__ rowptr, int32_t* __restrict__ out)
{
  AGG_FOR(r, nrows)
  {
    const int32_t len = (int32_t)(rowptr[r + 1] - rowptr[r]);
    atomicMax(&out[0], len);
    if (len == 0)
      atomicAdd(&out[1], 1);
  }
}

// r_c = P^T r_f in gather form: a thread per aggregate sums its members in ascending index -- no atomics, the same bits in
// every run.  sub != null: r_f = b - sub formed on the way in, as k_mg_restrict does.
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_restrict(const int* __restrict__ stop, int64_t nagg, const int32_t* __restrict__ moff,
                                                     const int32_t* __restrict__ mem, const uint8_t* __restrict__ bcf,
                                                     const double* __restrict__ rf, const double* __restrict__ sub,
                                                     double* __restrict__ rc)
{
  if (stop && *stop)
    return;
  AGG_FOR(a, nagg)
  {
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (int32_t t = moff[a]; t < moff[a + 1]; ++t)
    {
      const int64_t i = (int64_t)mem[t] * BS;
      {
        double v = sub ? rf[i] - sub[i] : rf[i];
        if (bcf[i])
          v = 0.0;
        acc0 += v;
      }
      if (BS == 3)
      {
        double v = sub ? rf[i + 1] - sub[i + 1] : rf[i + 1];
        if (bcf[i + 1])
          v = 0.0;
        acc1 += v;
        v = sub ? rf[i + 2] - sub[i + 2] : rf[i + 2];
        if (bcf[i + 2])
          v = 0.0;
        acc2 += v;
      }
    }
    rc[a * BS] = acc0;
    if (BS == 3)
    {
      rc[a * BS + 1] = acc1;
      rc[a * BS + 2] = acc2;
    }
  }
}

// x_f (+)= P e_c: one gather per fine scalar dof (at a clamped index where P's row is zero)
template <int BS>
__global__ __launch_bounds__(VB) void k_agg_prolong(const int* __restrict__ stop, int64_t nscalar, const int32_t* __restrict__ agg,
                                                    const uint8_t* __restrict__ bcf, const double* __restrict__ ec,
                                                    double* __restrict__ xf, int accumulate)
{
  if (stop && *stop)
    return;
  AGG_FOR(d, nscalar)
  {
    const int32_t a = agg[d / BS];
    const double e = ec[(int64_t)(a >= 0 ? a : 0) * BS + d % BS];
    const double s = (a < 0 || bcf[d]) ? 0.0 : e;
    xf[d] = accumulate ? xf[d] + s : s;
  }
}

AggLevel* agg_new() { return new AggLevel(); }
void agg_free(AggLevel* A) { delete A; }
int64_t agg_count(const AggLevel* A) { return A->nagg; }
const int32_t* agg_map(const AggLevel* A) { return A->agg.p; }
const int32_t* agg_member_offsets(const AggLevel* A) { return A->moff.p; }
const int32_t* agg_members(const AggLevel* A) { return A->mem.p; }

// flags (caller order) -> numbers base + rank for the flagged nodes; *count = how many
static int agg_number(zzz_ctx* ctx, AggLevel& A, int what, int32_t base, const int32_t* perm, const int32_t* state,
                      DevBuf<int32_t>& flag, DevBuf<int32_t>& scan, DevBuf<unsigned char>& tmp, int32_t* count)
{
  hipStream_t s = ctx->stream;
  const int64_t n = A.nf;
  const int g = grid_cap(n, VB, 1 << 16);
  hipLaunchKernelGGL(k_agg_flags, dim3(g), dim3(VB), 0, s, n, what, perm, state, A.agg.p, flag.p);
  if (int rc = with_scratch(ctx, tmp, scan_excl(flag.p, scan.p, (size_t)n + 1, s)))
    return rc;
  ZZZ_HIP(ctx, dev_fetch(ctx, scan.p + n, count));
  hipLaunchKernelGGL(k_agg_number, dim3(g), dim3(VB), 0, s, n, what, base, perm, flag.p, scan.p, A.agg.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return ZZZ_OK;
}

// The graph the aggregates are chosen on: n nodes of BS scalar rows each of a CSR matrix as it stands (pattern, zero structure
// of the values), the Dirichlet bytes of its scalar rows, and the nodes' numbers in the caller's numbering (null: their own).
struct AggGraph
{
  int64_t n;
  const rp_t* rowptr;
  const int32_t* cols;
  const double* vals;
  const uint8_t* bc;
  const int32_t* perm;
};

// The aggregates of that graph, on ctx->stream.
template <int BS>
static int agg_aggregate_bs(zzz_ctx* ctx, const AggGraph& G, AggLevel& A)
{
  hipStream_t s = ctx->stream;
  const int64_t n = G.n;
  const int g = grid_cap(n, VB, 1 << 16);
  const int32_t* perm = G.perm;
  A.bs = BS;
  A.nf = n;
  A.nagg = 0;
  DevBuf<int32_t> state, flag, scan, agg2, counter;
  DevBuf<long long> key, m1;
  DevBuf<uint8_t> near;
  DevBuf<unsigned char> tmp;
  ZZZ_HIP(ctx, state.alloc((size_t)n));
  ZZZ_HIP(ctx, flag.alloc((size_t)n + 1));
  ZZZ_HIP(ctx, scan.alloc((size_t)n + 1));
  ZZZ_HIP(ctx, agg2.alloc((size_t)n));
  ZZZ_HIP(ctx, counter.alloc(1));
  ZZZ_HIP(ctx, key.alloc((size_t)n));
  ZZZ_HIP(ctx, m1.alloc((size_t)n));
  ZZZ_HIP(ctx, near.alloc((size_t)n));
  ZZZ_HIP(ctx, A.agg.alloc((size_t)n));
  hipLaunchKernelGGL(k_agg_init<BS>, dim3(g), dim3(VB), 0, s, n, G.bc, perm, state.p, key.p);
  const rp_t* rp = G.rowptr;
  const int32_t* cl = G.cols;
  const double* vl = G.vals;
  A.rounds = 0;
  for (;;)
  {
    int32_t left = 0;
    ZZZ_HIP(ctx, hipMemsetAsync(counter.p, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_agg_max1<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, state.p, key.p, m1.p);
    hipLaunchKernelGGL(k_agg_max2<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, key.p, m1.p, state.p);
    hipLaunchKernelGGL(k_agg_near1<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, state.p, near.p);
    hipLaunchKernelGGL(k_agg_near2<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, near.p, state.p, counter.p);
    ZZZ_HIP(ctx, dev_fetch(ctx, counter.p, &left));
    ++A.rounds;
    if (left == 0)
      break;
    // (every round with an undecided node makes its largest one a root: the loop ends; the cap guards a broken matrix)
    if (A.rounds >= 4096)
      return fail(ctx, ZZZ_ERR_ARG, "-pc_type agg: the independent set did not close in %d rounds (%d nodes undecided)", A.rounds, left);
  }
  int32_t nroots = 0, nsingle = 0;
  if (int rc = agg_number(ctx, A, 0, 0, perm, state.p, flag, scan, tmp, &nroots))
    return rc;
  hipLaunchKernelGGL(k_agg_join<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, state.p, A.agg.p, agg2.p);
  hipLaunchKernelGGL(k_agg_join<BS>, dim3(g), dim3(VB), 0, s, n, rp, cl, vl, state.p, agg2.p, A.agg.p);
  if (int rc = agg_number(ctx, A, 1, nroots, perm, state.p, flag, scan, tmp, &nsingle))
    return rc;
  A.nagg = (int64_t)nroots + nsingle;
  // the map inverted: nodes in the caller's order, stably sorted by aggregate
  DevBuf<uint32_t> mk, mk2;
  DevBuf<int32_t> mv;
  ZZZ_HIP(ctx, mk.alloc((size_t)n));
  ZZZ_HIP(ctx, mk2.alloc((size_t)n));
  ZZZ_HIP(ctx, mv.alloc((size_t)n));
  ZZZ_HIP(ctx, A.mem.alloc((size_t)n));
  ZZZ_HIP(ctx, A.moff.alloc((size_t)A.nagg + 1));
  hipLaunchKernelGGL(k_agg_member_keys, dim3(g), dim3(VB), 0, s, n, perm, A.agg.p, mk.p, mv.p);
  if (int rc = with_scratch(ctx, tmp, sort_pairs(mk.p, mk2.p, mv.p, A.mem.p, (size_t)n, 0, 32, s)))
    return rc;
  hipLaunchKernelGGL((k_agg_offsets<uint32_t, int32_t>), dim3(g), dim3(VB), 0, s, mk2.p, n, A.nagg, A.moff.p);
  ZZZ_HIP(ctx, hipGetLastError());
  ZZZ_HIP(ctx, hipStreamSynchronize(s)); // (the scratch above is freed on return)
  return ZZZ_OK;
}

int agg_aggregate(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A)
{
  if (f->n_owned >= ((int64_t)1 << 31) / 4 || f->nnz >= (int64_t)INT32_MAX - 16)
    return fail(ctx, ZZZ_ERR_LIMIT, "-pc_type agg: %lld block dofs / %lld nonzeros on a level: 32-bit entry indices",
                (long long)f->n_owned, (long long)f->nnz);
  const AggGraph G{f->n_owned, f->rowptr.p, f->cols.p, f->vals.p, f->bc.p, f->dofmap.renumbered ? f->perm.p : nullptr};
  return f->bs == 3 ? agg_aggregate_bs<3>(ctx, G, *A) : agg_aggregate_bs<1>(ctx, G, *A);
}

// ... of a graph given as it is: one row per node (ZZZ_PC_SAGG_RBM's coarse levels: the nodes are blocks of six scalar rows of
// a matrix adopted as scalar, zzz_sagg.hip writes the node rows out)
int agg_aggregate_graph(zzz_ctx* ctx, int64_t n, int64_t nnz, const rp_t* rowptr, const int32_t* cols, const double* vals,
                        const uint8_t* bc, AggLevel* A)
{
  if (n >= ((int64_t)1 << 31) / 4 || nnz >= (int64_t)INT32_MAX - 16)
    return fail(ctx, ZZZ_ERR_LIMIT, "-pc_type agg: %lld nodes / %lld nonzeros on a level: 32-bit entry indices", (long long)n,
                (long long)nnz);
  return agg_aggregate_bs<1>(ctx, AggGraph{n, rowptr, cols, vals, bc, nullptr}, *A);
}

// The coarse values on the kept aggregates, and the product stream of the coarse context packed from them
int agg_refresh(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A, zzz_ctx* c)
{
  if (A->nnzc > 0)
    hipLaunchKernelGGL(k_agg_values, dim3(grid_cap(A->nnzc, VB, 1 << 16)), dim3(VB), 0, ctx->stream, A->nnzc, A->seg.p, A->src.p, f->vals.p, c->vals.p);
  ZZZ_HIP(ctx, hipGetLastError());
  return ctx_adopt_values(c);
}

// A_c = P^T A P into the child context c, which adopts it (pattern and values built here, on the device)
template <int BS>
static int agg_galerkin_bs(zzz_ctx* ctx, zzz_ctx* f, AggLevel& A, zzz_ctx* c)
{
  hipStream_t s = ctx->stream;
  const int64_t N = f->nnz, nrows = f->n_owned * BS, ncdof = A.nagg * BS;
  const int g = grid_cap(N, VB, 1 << 16);
  DevBuf<int32_t> rowidx, v0, v1, head, pos, crow, stats;
  DevBuf<unsigned long long> k0, k1;
  DevBuf<unsigned char> tmp;
  ZZZ_HIP(ctx, rowidx.alloc((size_t)N));
  ZZZ_HIP(ctx, v0.alloc((size_t)N));
  ZZZ_HIP(ctx, v1.alloc((size_t)N));
  ZZZ_HIP(ctx, k0.alloc((size_t)N));
  ZZZ_HIP(ctx, k1.alloc((size_t)N));
  ZZZ_HIP(ctx, head.alloc((size_t)N + 1));
  ZZZ_HIP(ctx, pos.alloc((size_t)N + 1));
  ZZZ_HIP(ctx, stats.alloc(2));
  ZZZ_HIP(ctx, A.src.alloc((size_t)N));
  hipLaunchKernelGGL(k_agg_rowidx, dim3(grid_cap(nrows, VB, 1 << 16)), dim3(VB), 0, s, nrows, f->rowptr.p, rowidx.p);
  const int32_t* order = nullptr;
  if (f->dofmap.renumbered)
  {
    hipLaunchKernelGGL(k_agg_caller_keys<BS>, dim3(g), dim3(VB), 0, s, N, rowidx.p, f->cols.p, f->perm.p, k0.p, v0.p);
    if (int rc = with_scratch(ctx, tmp, sort_pairs(k0.p, k1.p, v0.p, v1.p, (size_t)N, 0, 64, s)))
      return rc;
    order = v1.p;
  }
  // (v0 may be written while v1 is read: different buffers)
  hipLaunchKernelGGL(k_agg_coarse_keys<BS>, dim3(g), dim3(VB), 0, s, N, order, rowidx.p, f->cols.p, f->bc.p, A.agg.p, k0.p, v0.p);
  if (int rc = with_scratch(ctx, tmp, sort_pairs(k0.p, k1.p, v0.p, A.src.p, (size_t)N, 0, 64, s)))
    return rc;
  hipLaunchKernelGGL(k_agg_heads, dim3(g), dim3(VB), 0, s, N, k1.p, head.p);
  if (int rc = with_scratch(ctx, tmp, scan_excl(head.p, pos.p, (size_t)N + 1, s)))
    return rc;
  int32_t nnzc = 0;
  ZZZ_HIP(ctx, dev_fetch(ctx, pos.p + N, &nnzc));
  if (nnzc <= 0)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type agg: the coarse matrix of %lld aggregates is empty", (long long)A.nagg);
  A.nfine = N;
  A.nnzc = nnzc;
  ZZZ_HIP(ctx, A.seg.alloc((size_t)nnzc + 1));
  ZZZ_HIP(ctx, crow.alloc((size_t)nnzc));
  ZZZ_HIP(ctx, c->rowptr.alloc((size_t)ncdof + 1));
  ZZZ_HIP(ctx, c->cols.alloc((size_t)nnzc + 8));
  ZZZ_HIP(ctx, c->vals.alloc((size_t)nnzc + 8));
  ZZZ_HIP(ctx, hipMemsetAsync(c->cols.p + nnzc, 0, 8 * sizeof(int32_t), s));
  ZZZ_HIP(ctx, hipMemsetAsync(c->vals.p + nnzc, 0, 8 * sizeof(double), s));
  ZZZ_HIP(ctx, hipMemsetAsync(stats.p, 0, 2 * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_agg_entries, dim3(g), dim3(VB), 0, s, N, (int64_t)nnzc, k1.p, head.p, pos.p, A.seg.p, c->cols.p, crow.p);
  hipLaunchKernelGGL((k_agg_offsets<int32_t, rp_t>), dim3(grid_cap(nnzc, VB, 1 << 16)), dim3(VB), 0, s, crow.p, (int64_t)nnzc, ncdof, c->rowptr.p);
  hipLaunchKernelGGL(k_agg_values, dim3(grid_cap(nnzc, VB, 1 << 16)), dim3(VB), 0, s, (int64_t)nnzc, A.seg.p, A.src.p, f->vals.p, c->vals.p);
  hipLaunchKernelGGL(k_agg_rowstats, dim3(grid_cap(ncdof, VB, 1 << 16)), dim3(VB), 0, s, ncdof, c->rowptr.p, stats.p);
  int32_t hs[2] = {0, 0};
  ZZZ_HIP(ctx, dev_fetch(ctx, stats.p, hs, 2));
  ZZZ_HIP(ctx, hipGetLastError());
  if (hs[1] > 0)
    return fail(ctx, ZZZ_ERR_ARG, "-pc_type agg: %d coarse dofs have no unconstrained member (aggregates of partly constrained "
                                  "block dofs): the coarse matrix would be singular", hs[1]);
  if (int rc = ctx_adopt_csr(c, BS, A.nagg, nnzc, hs[0]))
    return fail(ctx, rc, "-pc_type agg: the coarse level of %lld dofs: %s", (long long)ncdof, c->err.c_str());
  return ZZZ_OK;
}

int agg_galerkin(zzz_ctx* ctx, zzz_ctx* f, AggLevel* A, zzz_ctx* c)
{
  return f->bs == 3 ? agg_galerkin_bs<3>(ctx, f, *A, c) : agg_galerkin_bs<1>(ctx, f, *A, c);
}

int agg_restrict(zzz_ctx* ctx, const int* stop, const AggLevel* A, const uint8_t* bcf, const double* rf, const double* sub, double* rc)
{
  const int g = grid_cap(A->nagg, VB, 1 << 16);
  if (A->bs == 3)
    hipLaunchKernelGGL(k_agg_restrict<3>, dim3(g), dim3(VB), 0, ctx->stream, stop, A->nagg, A->moff.p, A->mem.p, bcf, rf, sub, rc);
  else
    hipLaunchKernelGGL(k_agg_restrict<1>, dim3(g), dim3(VB), 0, ctx->stream, stop, A->nagg, A->moff.p, A->mem.p, bcf, rf, sub, rc);
  return ZZZ_OK;
}

int agg_prolong(zzz_ctx* ctx, const int* stop, const AggLevel* A, const uint8_t* bcf, const double* ec, double* xf, int accumulate)
{
  const int64_t n = A->nf * A->bs;
  const int g = grid_cap(n, VB, 1 << 16);
  if (A->bs == 3)
    hipLaunchKernelGGL(k_agg_prolong<3>, dim3(g), dim3(VB), 0, ctx->stream, stop, n, A->agg.p, bcf, ec, xf, accumulate);
  else
    hipLaunchKernelGGL(k_agg_prolong<1>, dim3(g), dim3(VB), 0, ctx->stream, stop, n, A->agg.p, bcf, ec, xf, accumulate);
  return ZZZ_OK;
}
ZZZ_PRELOAD_TU(agg)
} // namespace zzz
