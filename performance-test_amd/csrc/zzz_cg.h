// What the CG translation units share (zzz_cg.hip: classical, single-reduction, Chebyshev-Jacobi and multigrid forms;
// zzz_cg_pipe.hip: the pipelined form; zzz_cg_f32.hip: linalg::cg in float): the vector kernels' launch shape and load
// policy, the coded inverse diagonal, the partial-sum tree, and the host side every form's driver has in common --
//   CgSolve          the skeleton of a solve: prologue (histories, CgState, profile events), the timing of the product,
//                    the host's poll of the device state, and the epilogue (state read-back, iteration count, norms,
//                    history, profile averages, KSPConvergedReason)
//   cg_report_reset  what zzz_cg_info says about a solve, at its "nothing special" values
//   ChebPlan, cheb_first, cheb_terms   the Chebyshev-Jacobi polynomial: preconditioner and multigrid smoother
// Not part of the ABI.
#pragma once
#include "zzz_device.h"
#include "zzz_internal.h"

#include <type_traits>

namespace zzz
{
// One workgroup-wide sum of up to three partial arrays in ONE pass and one barrier pair (same tree per array as
// reduce_parts_bcast of zzz_cg.hip:
// strided per-thread sums, shuffles inside a wavefront, the per-wavefront sums added in order -- here by every thread
// from LDS instead of by thread 0 plus a broadcast).  pc may be null.
__device__ inline void reduce_parts3_bcast(const double* __restrict__ pa, const double* __restrict__ pb,
                                           const double* __restrict__ pc, int np, double& ra, double& rb, double& rc)
{
  __shared__ double sh[3 * 16];
  double s0 = 0, s1 = 0, s2 = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x)
  {
    s0 += pa[i];
    s1 += pb[i];
    if (pc)
      s2 += pc[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    s0 += __shfl_down(s0, o, 64);
    s1 += __shfl_down(s1, o, 64);
    s2 += __shfl_down(s2, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0)
  {
    sh[wv] = s0;
    sh[nw + wv] = s1;
    sh[2 * nw + wv] = s2;
  }
  __syncthreads();
  ra = rb = rc = 0.0;
  for (int i = 0; i < nw; ++i)
  {
    ra += sh[i];
    rb += sh[nw + i];
    rc += sh[2 * nw + i];
  }
}

constexpr int VB = 256;        // threads per workgroup of the vector kernels
constexpr int VGRID_MAX = 2048; // 8 workgroups per CU

// Product launches timed with HIP events when zzz_solver_opts.profile is set: every PROF_STRIDE-th iteration.  An event
// record between two kernels costs ~3.5 us of idle GPU (rocprofv3 timeline at 1.25 M rows: 4.1-4.4 us gaps on both sides
// of the product against 0.5-0.8 us elsewhere), i.e. 7 us per timed iteration -- 13 % of a 52-us iteration when every
// launch was timed.
constexpr int PROF_STRIDE = 8;

// The convergence flag can be set by workgroup 0 of the SAME launch while other workgroups start: one value per
// workgroup (thread 0's, loaded by the caller ahead of its other requests), so all threads of a workgroup take the same
// branch -- the reductions behind it need every wavefront.
__device__ inline int block_flag(int f)
{
  __shared__ int flag;
  if (threadIdx.x == 0)
    flag = f;
  __syncthreads();
  return flag;
}

struct DinvCodes
{
  const uint32_t* codes; // two 16-bit codes per word, entry pairs as the dbl2 accesses take them; bits == 8: one byte per entry
  const double* dict;
  const double* r;
  int ndict;
  int bits; // 16, or 8 when ndict <= DZ8_MAX (dinv_codes_build)
};
constexpr int DZ_MAX = 2048;
constexpr int DZ8_MAX = 256;

// The kernels that take DinvCodes are compiled per form of the inverse diagonal, their template parameter DZ: 0 doubles,
// 1 16-bit codes, 2 8-bit codes (the LDS table then holds DZ8_MAX entries).  One __global__ entry point per kernel; the
// host turns the load policy and dz_form() into its template arguments with dz_dispatch.  A dbl2 access' two codes are
// one load either way.
constexpr int dz_table(int DZ) { return DZ == 2 ? DZ8_MAX : DZ == 1 ? DZ_MAX : 1; }
inline int dz_form(const DinvCodes& dz) { return !dz.codes ? 0 : dz.bits == 8 ? 2 : 1; }
// f(std::integral_constant<bool, NT>, std::integral_constant<int, DZ>) for the pair that (nt, form) name
template <typename F>
auto dz_dispatch(bool nt, int form, F f)
{
  auto by_form = [&](auto NT) {
    return form == 2   ? f(NT, std::integral_constant<int, 2>{})
           : form == 1 ? f(NT, std::integral_constant<int, 1>{})
                       : f(NT, std::integral_constant<int, 0>{});
  };
  return nt ? by_form(std::true_type{}) : by_form(std::false_type{});
}
// the dictionary into the kernel's LDS table (dtab[dz_table(DZ)]), by the whole workgroup
template <int DZ>
__device__ __forceinline__ void dz_stage(double (&dtab)[dz_table(DZ)], const DinvCodes& dz)
{
  if (DZ)
  {
    for (int k = threadIdx.x; k < dz.ndict; k += VB)
      dtab[k] = dz.dict[k];
    __syncthreads();
  }
}
template <int DZ>
__device__ inline uint32_t dz_load2(const DinvCodes& dz, int64_t i2) // the codes of entries 2 i2 and 2 i2 + 1
{
  return DZ == 2 ? (uint32_t)reinterpret_cast<const uint16_t*>(dz.codes)[i2] : dz.codes[i2];
}
template <int DZ>
__device__ inline uint32_t dz_lo(uint32_t dc)
{
  return DZ == 2 ? dc & 0xffu : dc & 0xffffu;
}
template <int DZ>
__device__ inline uint32_t dz_hi(uint32_t dc)
{
  return DZ == 2 ? dc >> 8 : dc >> 16;
}
template <int DZ>
__device__ inline uint32_t dz_load1(const DinvCodes& dz, int64_t i) // the code of entry i
{
  return DZ == 2 ? (uint32_t)reinterpret_cast<const uint8_t*>(dz.codes)[i] : (uint32_t)reinterpret_cast<const uint16_t*>(dz.codes)[i];
}

// the polling events of one solve: destroyed on every exit path
template <int N>
struct EventRing
{
  hipEvent_t ev[N] = {};
  int created = 0;
  hipError_t create()
  {
    for (; created < N; ++created)
    {
      hipError_t e = hipEventCreateWithFlags(&ev[created], hipEventDisableTiming);
      if (e != hipSuccess)
        return e;
    }
    return hipSuccess;
  }
  ~EventRing()
  {
    for (int i = 0; i < created; ++i)
      (void)hipEventDestroy(ev[i]);
  }
  hipEvent_t& operator[](int i) { return ev[i]; }
};

// The skeleton of one solve.  A driver keeps its own loop and launches and calls, in this order: begin() AFTER its
// preconditioner's set-up (chebyshev_setup and mg_setup run a solve of their own through the same context) and before its
// first stream operation; per iteration product_begin() / product_end() around the product and poll() at the end;
// finish() behind its last launch.
struct CgSolve
{
  // host polling: copy the state every CHECK iterations, look at it NSLOT-1 batches later
  static constexpr int CHECK = 8, NSLOT = 4;
  zzz_ctx* ctx = nullptr;
  const zzz_solver_opts* o = nullptr;
  int stride = PROF_STRIDE; // every stride-th product is timed (zzz_solver_opts.profile)
  int max_prof = 0, nprof = 0, nchk = 0;
  bool timed = false;
  bool stop = false; // set by poll(): the device had stopped in the copy looked at
  EventRing<NSLOT> chk_ev;

  // beta_hist and dp_hist reserved (a form's other buffers are its own), CgState cleared on the stream, profile events
  // made, halo-wait samples reset, polling events made
  int begin(zzz_ctx* c, const zzz_solver_opts* opts, int prof_stride = PROF_STRIDE);
  void product_begin(int it); // it: the loop's counter
  int product_end(int rc);    // rc: the product's return code, handed back (prof_now is cleared either way)
  int poll(int done);         // done: iterations enqueued so far
  // behind the last launch: waits for the stream; last_iters, *iters, rnorm[0..1], the history, the profile's means,
  // last_reason.  ZZZ_ERR_DIVERGED only under error_if_not_converged.
  int finish(int* iters, double* rnorm);
};

// The Chebyshev-Jacobi polynomial x = p_k(D^-1 A) D^-1 b for D^-1 A on [lo, hi] = [hi / ratio, hi]: the preconditioner
// of ZZZ_PC_CHEBYSHEV_JACOBI and the smoother of every multigrid level.  Its constants, its work vectors (nloc doubles
// each, of the context whose operator it applies) and the form of its terms.
struct ChebPlan
{
  int degree = 0;
  double hi = 0.0, lo = 0.0, theta = 0.0, delta = 0.0, sigma = 0.0;
  double *g = nullptr, *d = nullptr, *d2 = nullptr; // residual of the polynomial's recurrence; its direction, two buffers
  // terms as epilogues of their products (ChebEpi) instead of launches of their own: chebyshev_setup says where the
  // product allows it; ZZZ_PC_CHEBYSHEV_JACOBI on the caller's context takes that, a multigrid level declines
  bool fused = false;
  ChebPlan() = default;
  ChebPlan(double hi_, double ratio, int degree_)
      : degree(degree_), hi(hi_), lo(hi_ / ratio), theta(0.5 * (hi + lo)), delta(0.5 * (hi - lo)), sigma(theta / delta)
  {
  }
  // the coefficients of the next term, d_j = c1 d_(j-1) + c2 g; rho starts at 1 / sigma (the first term's) and is advanced
  void next_term(double& rho, double& c1, double& c2) const
  {
    const double rhon = 1.0 / (2.0 * sigma - rho);
    c1 = rhon * rho;
    c2 = 2.0 * rhon / delta;
    rho = rhon;
  }
};
// The polynomial on context c (operator, inverse diagonal, n_owned * bs entries), enqueued on owner's stream and skipped
// once owner's CgState says stop (owner is c or the context whose hierarchy c is a level of).
//   cheb_first: g = D^-1 (b - t) or, t == null, D^-1 b (the start from zero: no product);  d = g / theta;  x (+)= d
//   cheb_terms: terms 2 .. degree, a product of c each.  pa != null: the last one leaves g and d alone and sums the
//               partials of <b,x> and of the test norm -- into pa / pb (vgrid of them) when it is a launch of its own,
//               into the product's partial arrays at strides 1 and 2 (*np of them) when it is an epilogue
int chebyshev_setup(zzz_ctx* ctx, const zzz_solver_opts* o, ChebPlan& C); // the plan of o's degree and ratio for ctx's matrix
void cheb_first(zzz_ctx* c, zzz_ctx* owner, const ChebPlan& C, const double* b, const double* t, double* x);
int cheb_terms(zzz_ctx* c, zzz_ctx* owner, const ChebPlan& C, const double* b, double* x, int norm = 0, double* pa = nullptr,
               double* pb = nullptr, int* np = nullptr);

// zzz_cg.hip
void cg_report_reset(zzz_ctx* ctx); // last_pc_bound, last_solve_red_overlapped, last_solve_xdefer_k, last_solve_dinv_codes
// ctx->dinv as 8- or 16-bit codes (dzc.codes stays null: too many values)
int dinv_codes_build(zzz_ctx* ctx, int64_t n, DinvCodes& dzc);
bool loop_exceeds_cache(zzz_ctx* ctx, int nvec);               // operator + nvec vectors against the Infinity Cache
int vgrid(int64_t n);                                          // workgroups of a vector kernel over n entries
int cg_solve_pipe(zzz_ctx* ctx, const zzz_solver_opts* o, int* iters, double* rnorm); // zzz_cg_pipe.hip
// the start-up kernels on the context's stream: ctx->dinv = 1 / diag(A) (jacobi) or 1; r = b, z = dinv r with the
// partials of <r,z> and of the test norm
void cg_launch_extract_dinv(zzz_ctx* ctx, int64_t n, int jacobi);
void cg_launch_init_residual(zzz_ctx* ctx, double* z, int64_t n, int norm, double* pa, double* pb);
} // namespace zzz
