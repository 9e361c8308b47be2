// What zzz_sagg.hip (ZZZ_PC_SAGG) shares with zzz_sagg_rbm.hip (ZZZ_PC_SAGG_RBM): the stored prolongator of one level and the
// term lists behind its values and the two products, and the host steps that build them from a list of P's terms.  The two
// kinds differ in where P's terms come from and in P's value kernel; R = P^T, T = A P, A_c = P^T T, the refresh of their
// values and the two transfers are zzz_sagg.hip's for both.  (Not part of the ABI.)
#pragma once

#include "zzz_cg.h"

#include "zzz_prim.h"

namespace zzz
{
typedef unsigned long long u64;
constexpr u64 SAGG_NOKEY = ~0ull;
constexpr int RBM_NCOL = 6; // ZZZ_PC_SAGG_RBM: columns of P per aggregate, one per rigid-body mode

struct SaggLevel
{
  int bs = 1;
  const char* tag = "-pc_type sagg"; // of the messages
  int64_t nf = 0, nc = 0; // scalar dofs, fine and coarse
  AggLevel* agg = nullptr;
  // P: rows are the fine scalar dofs in the level's stored order; entry e sums the terms psrc[t] of its run (ZZZ_PC_SAGG: the
  // matrix entries psrc[t] >> 32; ZZZ_PC_SAGG_RBM: matrix entry psrc[t] >> 32 times entry psrc[t] & 0xffffffff of qt)
  int64_t pnnz = 0, pterms = 0;
  DevBuf<rp_t> prow;
  DevBuf<int32_t> pcol, pfrow, pseg;
  DevBuf<u64> psrc;
  DevBuf<double> pval, diag;
  // R = P^T: entry t of coarse row J is P's entry rsrc[t], of fine row rfine[t]
  DevBuf<rp_t> rrow;
  DevBuf<int32_t> rfine, rsrc;
  DevBuf<double> rval;
  // T = A P: entry e sums a[tsrc >> 32] * P[tsrc & 0xffffffff] over its run;  A_c: entry E sums T[csrc >> 32] * P[csrc & ...]
  // (pval and tval carry one more slot each, 1.0: the term of the unit diagonal of a dropped coarse dof is their product)
  int64_t tnnz = 0, cnnz = 0, tterms = 0, cterms = 0;
  DevBuf<int32_t> tseg, cseg;
  DevBuf<u64> tsrc, csrc;
  DevBuf<double> tval;
  // ZZZ_PC_SAGG_RBM alone (zzz_sagg_rbm.hip).  ns: scalar dofs per node of this level (3 on level 0, 6 below).  Member row
  // g = t ns + c is component c of node mem[t] of the aggregates' inverted map: the rows of an aggregate are contiguous.
  // qt[q nf + g]: column q of the aggregate's orthonormal basis Q in member row g -- P_t's values.  pos[node] = t.
  // B (level 0 alone: a coarse level reads the Bc of the level above): the near-nullspace the orthogonalisation read, [6][nf]
  // in the caller's numbering.  Bc: the next level's, [6][nc].  drop[d] = 1: coarse dof d is dropped; droplist: those, ascending.
  int ns = 0;
  int64_t ndrop = 0;
  DevBuf<double> qt, B, Bc;
  DevBuf<int32_t> pos, drop, droplist;
  // ZZZ_MG_PRODUCTS_ROWS (zzz_sagg_rows.hip): no term list.  P and R are the CSR above (pfrow, pseg, psrc, tseg, tsrc, cseg,
  // csrc stay empty); T is a CSR of its own, rows in the level's stored order; ord (level 0 in an internal order alone): the
  // matrix entries of every stored row in ascending caller column.  ri: what the last build's symbolic passes did.
  bool rows = false;
  DevBuf<rp_t> trow;
  DevBuf<int32_t> tcol, ord;
  struct RowsInfo
  {
    int64_t chunks = 0, max_cand = 0, budget = 0, lone = 0, peak = 0;
  } ri;
  ~SaggLevel() { agg_free(agg); }
};

#define SAGG_FOR(i, n) for (int64_t i = blockIdx.x * (int64_t)VB + threadIdx.x; i < (n); i += (int64_t)gridDim.x * VB)

// scalar dof d in the caller's numbering (perm: internal -> caller block index; null: the same)
template <int BS>
__device__ inline u64 sagg_caller(const int32_t* __restrict__ perm, int32_t d)
{
  return perm ? (u64)perm[d / BS] * BS + (unsigned)(d % BS) : (u64)d;
}

// the work buffers of the sorts of one level, freed together
struct SaggWork
{
  DevBuf<u64> k0, k1, v0;
  DevBuf<int32_t> head, pos, cnt;
  DevBuf<int64_t> off;
  DevBuf<unsigned char> tmp;
};

// what a level's term lists start from: the scalar row of every matrix entry of f, and the entries in ascending (row, column)
// of the caller's numbering (order null: as they are stored); perm null: f keeps the caller's numbering
struct SaggFrame
{
  SaggWork W;
  DevBuf<int32_t> rowidx;
  DevBuf<u64> ordbuf;
  const u64* order = nullptr;
  const int32_t* perm = nullptr;
};
int sagg_frame(zzz_ctx* ctx, zzz_ctx* f, SaggFrame& Fr);
// W.cnt[0 .. n] -> W.off (64-bit), *total; refused above the limit of 32-bit term positions (ZZZ_SAGG_MAX_TERMS lowers it);
// W.k0 / W.v0 take *total + extra terms
int sagg_term_offsets(zzz_ctx* ctx, const SaggLevel& S, SaggWork& W, int64_t n, int level, const char* what, int64_t extra,
                      int64_t* total);
// P's pattern, rows and runs from its n terms in Fr.W.k0 / v0: key (fine row << 32) | coarse column, SAGG_NOKEY: no term
int sagg_p_from_terms(zzz_ctx* ctx, SaggLevel& S, SaggFrame& Fr, int64_t n, int level);
// Writes n further terms of A_c (the unit diagonals of the dropped coarse dofs) behind the products' own: keys and values at
// key / val, every value `unit`
struct SaggUnitTerms
{
  int64_t n = 0;
  const int32_t* dofs = nullptr; // device: the coarse dofs, ascending
  void (*write)(hipStream_t s, int64_t n, const int32_t* dofs, u64 unit, u64* key, u64* val) = nullptr;
};
// R, T and A_c from P's pattern: their patterns and term lists; c's rowptr / cols / vals are allocated here.  *max_row = the
// longest row of A_c; a coarse dof with an empty row is refused.
int sagg_products(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c, int level, SaggFrame& Fr, const SaggUnitTerms& unit, int* max_row);
// a_ii of f's rows into S.diag;  then, with P's values in S.pval: R's, T's and A_c's (into c->vals) on the kept term lists
int sagg_diagonal(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S);
int sagg_product_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, zzz_ctx* c);
// R = P^T from P's pattern (S.prow / S.pcol; pfrow: the stored fine row of every entry of P): S.rrow, S.rfine, S.rsrc are
// filled and S.rval allocated; perm as SaggFrame's.  Both modes build R here.
int sagg_transpose_p(zzz_ctx* ctx, SaggLevel& S, const int32_t* perm, const int32_t* pfrow, SaggWork& W);
// pieces of the lists mode that the rows mode launches as they are: the row of every entry of a CSR; R's values from P's;
// out[0] = the longest row, out[1] = the empty rows of a CSR (out: two zeroed device words)
void sagg_row_index(zzz_ctx* ctx, int64_t nrows, const rp_t* rowptr, int32_t* rowidx);
void sagg_r_values(zzz_ctx* ctx, SaggLevel& S);
void sagg_row_stats(zzz_ctx* ctx, int64_t nrows, const rp_t* rowptr, int32_t* out);

// ---- ZZZ_MG_PRODUCTS_ROWS (zzz_sagg_rows.hip) ----------------------------------------------------------------------
// P_t as the row-by-row engine reads it: ZZZ_PC_SAGG's (one entry 1 per unconstrained dof of an aggregate) or
// ZZZ_PC_SAGG_RBM's (the kept columns of Q in S.qt)
enum class SaggPt
{
  UNIT,
  RBM
};
// P, R, T and A_c of level f in the rows mode, patterns and values; c's rowptr / cols / vals are allocated here.  The
// aggregates (and for RBM: S.qt, S.pos, S.drop, S.droplist, S.ndrop) stand.  *max_row = the longest row of A_c.
int sagg_rows_build(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, SaggPt pt, double omega, zzz_ctx* c, int level, int* max_row);
// the values again on the kept patterns: no sort, no allocation
int sagg_rows_values(zzz_ctx* ctx, zzz_ctx* f, SaggLevel& S, SaggPt pt, double omega, zzz_ctx* c);
} // namespace zzz
