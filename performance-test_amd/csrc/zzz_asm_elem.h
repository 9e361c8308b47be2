// What the row-gather assembly kernels of zzz_assemble.hip share (device code only): a cell's geometry, the entries of the
// element matrices, the column searches, the iteration over a row's cells, the P1 cell pipeline and the frame of a tile.
#pragma once

#include <climits>

#include "zzz_cell_geom.h"
#include "zzz_device.h"
#include "zzz_internal.h"

namespace zzz
{
constexpr int ASM_BLOCK = 256;
constexpr int ASM_ORD_CAP = 512; // block dofs of a tile that the high-order kernels sort by cell count

__device__ inline void load_cell(const double* __restrict__ x, const int4 v, double p[4][3])
{
  const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k)
  {
    const double* q = x + 3 * (int64_t)vv[k];
    p[k][0] = q[0];
    p[k][1] = q[1];
    p[k][2] = q[2];
  }
}

// P1 through the dof-addressed coordinates (zzz_ctx::xq): dd = the cell's four block dofs
__device__ inline void load_cell_q(const double* __restrict__ xq, const int4 dd, double p[4][3]) { load_cell(xq, dd, p); }
// the same for a row that knows its own vertex (local index li, coordinates own[]): three gathers instead of four.  The
// loads are predicated per lane; where the lanes of a wavefront agree on li (structured feeds) the fourth is not issued.
__device__ inline void load_cell_q3(const double* __restrict__ xq, const int4 dd, int li, const double own[3], double p[4][3])
{
  const int vv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
  for (int k = 0; k < 4; ++k)
  {
    if (k != li)
    {
      const double* q = xq + 3 * (int64_t)vv[k];
      p[k][0] = q[0];
      p[k][1] = q[1];
      p[k][2] = q[2];
    }
    else
    {
      p[k][0] = own[0];
      p[k][1] = own[1];
      p[k][2] = own[2];
    }
  }
}

// physical gradients of the four P1 hat functions: g[i][a] = sum_al K[al][a] * dphi_i/dX_al
__device__ inline void p1_grads(const Geom& G, double g[4][3])
{
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    g[1][a] = G.K[0][a];
    g[2][a] = G.K[1][a];
    g[3][a] = G.K[2][a];
    g[0][a] = -(G.K[0][a] + G.K[1][a] + G.K[2][a]);
  }
}

__device__ inline double sel3(double a0, double a1, double a2, int c) { return c == 0 ? a0 : (c == 1 ? a1 : a2); }

// ---- entries of the element matrices of form a, shared by the matrix kernels and the lifting pass (k_lift), so that
// the two cannot drift apart.  Every helper is the expression the matrix kernels held inline: same operations, same order.
constexpr double EL_E = 1.0e6, EL_NU = 0.3; // src/Elasticity.py:12-15
constexpr double EL_MU = EL_E / (2.0 * (1.0 + EL_NU));
constexpr double EL_LAMBDA = EL_E * EL_NU / ((1.0 + EL_NU) * (1.0 - 2.0 * EL_NU));

// P1 elasticity, entry (row node i, component c; column node j, component d) of a cell of reference volume weight w:
// mu (delta_cd g_i.g_j + d_d phi_i d_c phi_j) + lambda d_c phi_i d_d phi_j, with gg = g_i.g_j, gid = d_d phi_i,
// gjc = d_c phi_j, gic = d_c phi_i, gjd = d_d phi_j
__device__ inline double p1_elasticity_entry(double w, double gg, bool c_is_d, double gid, double gjc, double gic, double gjd)
{
  return w * (EL_MU * ((c_is_d ? gg : 0.0) + gid * gjc) + EL_LAMBDA * gic * gjd);
}

// Pk Poisson: |detJ| (K K^T) (six numbers: 00 11 22 01 02 12) contracted with the symmetrised reference tensors of the
// pair (li, j); Tlj points at piece 0 of the pair, the pieces are NN apart
template <int NN>
__device__ inline double pk_poisson_entry(const double* GG, const double* Tlj)
{
  double val = 0.0;
#pragma unroll
  for (int t = 0; t < 6; ++t)
    val += GG[t] * Tlj[t * NN];
  return val;
}

// Pk elasticity: D[cc][d] = |detJ| sum_{al,be} K[al][cc] K[be][d] S^[al][be]_{li,j} = int d_cc phi_i d_d phi_j
// (Kf: K[al][d] at Kf[3 al + d]; Tlj points at piece (0, 0) of the pair (li, j), the nine pieces are NN apart)
template <int NN>
__device__ inline void pk_grad_products(double adet, const double* Kf, const double* Tlj, double (&D)[3][3])
{
  double tmp[3][3];
#pragma unroll
  for (int al = 0; al < 3; ++al)
#pragma unroll
    for (int d = 0; d < 3; ++d)
      tmp[al][d] = Tlj[(al * 3 + 0) * NN] * Kf[0 + d] + Tlj[(al * 3 + 1) * NN] * Kf[3 + d] + Tlj[(al * 3 + 2) * NN] * Kf[6 + d];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc)
#pragma unroll
    for (int d = 0; d < 3; ++d)
      D[cc][d] = adet * (Kf[0 + cc] * tmp[0][d] + Kf[3 + cc] * tmp[1][d] + Kf[6 + cc] * tmp[2][d]);
}
// ... and the entry (component c of the row, d of the column) of the pair from D and its trace
__device__ inline double pk_elasticity_entry(const double (&D)[3][3], double tr, int c, int d)
{
  const double Dcd = sel3(D[0][d], D[1][d], D[2][d], c), Ddc = sel3(D[d][0], D[d][1], D[d][2], c);
  return EL_MU * ((c == d ? tr : 0.0) + Ddc) + EL_LAMBDA * Dcd;
}
// |detJ| (K K^T): 00 11 22 01 02 12
__device__ inline void pk_poisson_geom(const Geom& G, double (&GG)[6])
{
  GG[0] = G.adet * (G.K[0][0] * G.K[0][0] + G.K[0][1] * G.K[0][1] + G.K[0][2] * G.K[0][2]);
  GG[1] = G.adet * (G.K[1][0] * G.K[1][0] + G.K[1][1] * G.K[1][1] + G.K[1][2] * G.K[1][2]);
  GG[2] = G.adet * (G.K[2][0] * G.K[2][0] + G.K[2][1] * G.K[2][1] + G.K[2][2] * G.K[2][2]);
  GG[3] = G.adet * (G.K[0][0] * G.K[1][0] + G.K[0][1] * G.K[1][1] + G.K[0][2] * G.K[1][2]);
  GG[4] = G.adet * (G.K[0][0] * G.K[2][0] + G.K[0][1] * G.K[2][1] + G.K[0][2] * G.K[2][2]);
  GG[5] = G.adet * (G.K[1][0] * G.K[2][0] + G.K[1][1] * G.K[2][1] + G.K[1][2] * G.K[2][2]);
}

__device__ inline int find_pos(const int32_t* __restrict__ c, int len, int32_t col)
{
  int lo = 0, hi = len - 1;
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (c[mid] < col)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The positions of four columns in a row's sorted columns c[0 .. len): four lower-bound searches side by side, without
// branches -- pos = number of entries below the column, found bit by bit from the top.  (One after the other, as loops
// around find_pos, the four searches of a P1 cell were twenty dependent LDS round trips per (row, cell) pair, half of
// asm_matrix_p1's time; side by side they are five.)
__device__ inline void find_pos4(const int32_t* __restrict__ c, int len, const int (&col)[4], int (&pos)[4])
{
  // byte offsets from c: q = 4 pos; an entry is read at q + 4 step - 4 whether or not it lies in the row (the arrays this is
  // called on are 32 entries longer than the rows they hold) and counts only if it does
  const char* __restrict__ cb = reinterpret_cast<const char*>(c);
  const int end = 4 * len;
  int q[4] = {0, 0, 0, 0};
  int top = 16;
  while (top * 2 <= len) // (not taken on a P1 lattice: 27 columns at most)
    top *= 2;
  for (; top > 16; top >>= 1)
  {
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const int t = q[j] + 4 * top;
      const int v = t <= end ? *reinterpret_cast<const int32_t*>(cb + t - 4) : INT_MAX;
      q[j] = v < col[j] ? t : q[j];
    }
  }
  const bool short_rows = __all(len < 16); // (a P1 lattice of Kuhn simplices: 15 columns per row)
#pragma unroll
  for (int step = 64; step >= 4; step >>= 1) // 16 entries, 8, ... 1
  {
    if (step == 64 && short_rows)
      continue;
    int v[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      t[j] = q[j] + step;
      v[j] = *reinterpret_cast<const int32_t*>(cb + q[j] + (step - 4));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      q[j] = ((int)(t[j] <= end) & (int)(v[j] < col[j])) ? t[j] : q[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    pos[j] = q[j] >> 2;
}

// iteration over the cells of block dof i through the transposed adjacency (k_adjT_fill: entry a of row 64 s + lane sits at
// off[s] + 64 a + lane, cell index, -1 = padding, with the dof's local index in that cell beside it)
struct AdjIter
{
  const int32_t* cp;
  const uint8_t* lp;
  int len;
  __device__ AdjIter(const int32_t* __restrict__ off, const int32_t* __restrict__ cellT, const uint8_t* __restrict__ liT, int i)
  {
    const int sl = i >> 6, ln = i & 63;
    const int o = off[sl];
    len = (off[sl + 1] - o) >> 6;
    cp = cellT + o + ln;
    lp = liT + o + ln;
  }
  __device__ int cell(int a) const { return cp[a * 64]; } // -1 once the list of this row is exhausted
  __device__ int li(int a) const { return lp[a * 64]; }
};

// ---- the cell walk of the P1 matrix kernels (asm_matrix_p1: a lane per scalar row; asm_matrix_p1_node3: a lane per node)
// Three-stage software pipeline over the row's cells.  A cell needs a chain of three dependent loads (adjacency
// -> connectivity -> coordinates and BC flags); each link is issued one iteration ahead of the next: while cell a
// is evaluated the coordinates of a+1, the connectivity of a+2 and the adjacency entry a+3 are in flight, so an
// iteration waits for one memory round trip, not three (the workgroup's CSR segment in LDS leaves 3-4 wavefronts
// per SIMD: occupancy alone does not hide the chain).
// (profiles/r05_pmc_asm_c2.json, 10 M dofs: 296 VALU + 44 SALU + 26 LDS + 17 VMEM instructions per (row, cell) pair,
// VALU busy 78 % of the kernel's cycles, L2 hit rate 80 %: the kernel is bound by the instructions it issues -- with
// every gather, the search and the geometry removed (a timing probe, since removed from the code) it still takes 1.55 of its
// 2.65 ms: three wavefronts per SIMD, 24 dependent round trips per row.)
// The walk has no branches: every lane runs the slice's `alen` iterations (the transposed adjacency pads shorter
// rows with -1), a padding entry loads and evaluates cell 0 and only its update of the row is masked (body sees
// K.cell < 0); the coordinate stages alternate between two register sets (DA, DB: no copies of 25 registers per cell).
// Every load is unconditional, at a clamped index.
struct P1Conn
{
  int cell, li; // the cell (-1: padding) and the row's local index in it
  int4 dd;      // its four block dofs
};
template <int BS>
struct P1Data
{
  double p[4][3];      // the cell's vertices
  uint8_t bcj[4 * BS]; // Dirichlet flags of its columns
};

// body(K, D): the current cell's connectivity and data, in the row's adjacency order
template <int BS, class Body>
__device__ inline void p1_walk_cells(const AdjIter& adj, const double* __restrict__ xq, const int32_t* __restrict__ cell_dofs,
                                     const uint8_t* __restrict__ bc, Body&& body)
{
  using Conn = P1Conn;
  using Data = P1Data<BS>;
  const int alen = adj.len;
  auto adj_at = [&](int a, int& cell, int& li) {
    const int ac = min(a, alen - 1);
    const int cc = adj.cell(ac);
    cell = a < alen ? cc : -1;
    li = adj.li(ac);
  };
  auto conn_at = [&](int cell, int li, Conn& K) {
    K.cell = cell;
    K.li = li;
    K.dd = *reinterpret_cast<const int4*>(cell_dofs + 4 * (int64_t)max(cell, 0));
  };
  auto data_at = [&](const Conn& K, Data& D) {
    load_cell_q(xq, K.dd, D.p); // (skipping the row's own vertex, as asm_vector_p1 does, made asm_matrix_p1 3 % slower)
    const int dj[4] = {K.dd.x, K.dd.y, K.dd.z, K.dd.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int d = 0; d < BS; ++d)
        D.bcj[j * BS + d] = bc[dj[j] * BS + d];
  };
  Conn K0, K1;
  Data DA, DB;
  int c2, l2;
  auto iter = [&](int a, const Data& D0, Data& D1) {
    Conn K2;
    int c3, l3;
    data_at(K1, D1);
    conn_at(c2, l2, K2);
    adj_at(a + 3, c3, l3);
    body(K0, D0);
    K0 = K1;
    K1 = K2;
    c2 = c3;
    l2 = l3;
  };
  if (alen > 0)
  {
    {
      int ca, la;
      adj_at(0, ca, la);
      conn_at(ca, la, K0);
      data_at(K0, DA);
      adj_at(1, ca, la);
      conn_at(ca, la, K1);
      adj_at(2, c2, l2);
    }
    int a = 0;
    for (; a + 1 < alen; a += 2)
    {
      iter(a, DA, DB);
      iter(a + 1, DB, DA);
    }
    if (a < alen)
      iter(a, DA, DB);
  }
}

// ---- the frame of a tile in the matrix kernels: block dofs [d0, d1) = scalar rows [row0, row1), whose CSR segment
// starts at s and has e entries (it fits LDS: asm_tile_nnz)
struct TileSpan
{
  int d0, d1, row0, row1;
  int64_t s;
  int e;
};
template <int BS>
__device__ inline TileSpan tile_span(const int32_t* __restrict__ tiles, const rp_t* __restrict__ rowptr, int64_t tile)
{
  TileSpan t;
  t.d0 = tiles[tile];
  t.d1 = tiles[tile + 1];
  t.row0 = t.d0 * BS;
  t.row1 = t.d1 * BS;
  t.s = rowptr[t.row0];
  t.e = (int)(rowptr[t.row1] - t.s);
  return t;
}

// The reference tensors of element_tables.inc that form a is contracted with, into T_s (NT * ND * ND doubles, NT = 6 for
// BS = 1, 9 for BS = 3), by a workgroup of ASM_BLOCK threads; the caller places the barrier.  BS = 1: the symmetrised
// pieces 00 11 22 01 02 12 -- G is symmetric, so S^{ab} + S^{ba} is all a < b needs.
template <int ND, int BS>
__device__ inline void stage_reference_tensors(const double* __restrict__ tab, double* T_s)
{
  constexpr int NT = (BS == 1) ? 6 : 9;
  constexpr int NN = ND * ND;
  for (int k = threadIdx.x; k < NT * NN; k += ASM_BLOCK)
  {
    if (BS == 1)
    {
      const int t = k / NN, ij = k % NN;
      const int a = t < 3 ? t : (t == 3 ? 0 : (t == 4 ? 0 : 1)), b = t < 3 ? t : (t == 3 ? 1 : 2);
      T_s[k] = (t < 3) ? tab[(a * 3 + a) * NN + ij] : tab[(a * 3 + b) * NN + ij] + tab[(b * 3 + a) * NN + ij];
    }
    else
      T_s[k] = tab[k];
  }
}

// Block dofs d0 .. d0 + nt of a tile in order of descending cell count (counting sort in LDS: ord_s[ASM_ORD_CAP],
// hist_s[34]): with the point-major numbering a tile mixes vertex rows (24 cells) with face rows (2 cells), and a
// wavefront takes as long as its heaviest row.  Which lane group computes a row changes nothing in the result.
// Returns false, ord_s untouched, for a tile of more than ASM_ORD_CAP block dofs; the caller places the barrier
// behind the last writes of ord_s.
__device__ inline bool tile_order_by_cell_count(const int32_t* __restrict__ adj_off, int d0, int nt, int* ord_s, int* hist_s)
{
  if (nt > ASM_ORD_CAP)
    return false;
  if (threadIdx.x < 34)
    hist_s[threadIdx.x] = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < nt; k += ASM_BLOCK)
    atomicAdd(&hist_s[32 - min(adj_off[d0 + k + 1] - adj_off[d0 + k], 32)], 1);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    int acc = 0;
    for (int b = 0; b < 33; ++b)
    {
      const int h = hist_s[b];
      hist_s[b] = acc;
      acc += h;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nt; k += ASM_BLOCK)
    ord_s[atomicAdd(&hist_s[32 - min(adj_off[d0 + k + 1] - adj_off[d0 + k], 32)], 1)] = k;
  return true;
}
} // namespace zzz
