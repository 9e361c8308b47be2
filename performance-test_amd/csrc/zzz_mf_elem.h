// Per-cell arithmetic of the matrix-free action (zzz_matfree.hip) and the rounding rules of its single-precision value
// arrays, generic over the scalar R as src/cgpoisson_problem.cpp:28 (`using T = PetscScalar`) makes the reference's.
// Host-compilable (as zzz_pmg.h is): a stand-alone program runs the same code on the CPU under the sanitizers.
//   * geometry factors, reference tables: computed in double, then rounded once (mf_round);
//   * P1 coordinates: NOT absolute.  The Jacobian is a difference of coordinates; formed from rounded absolute values its
//     relative error is eps32 / h and grows with the mesh.  The float copy holds every coordinate relative to an origin of
//     its cell block, subtracted in double (mf_rel_coord).  A rounded relative coordinate is off by 2^-25 of its DISTANCE
//     FROM THE ORIGIN, so an entry of a cell's Jacobian is off by up to 2^-24 x (distance from the origin) / (the cell's
//     extent along that axis): harmless where a block spans a few dozen of its cells, ruinous on a graded mesh whose block
//     holds cells 10^5 times smaller than itself far from its origin (the far cells collapse to det J == 0 in float).  So
//     the origin is CHECKED, cell by cell (mf_f32_cell), a second origin is tried (MfF32Thin) and a block neither origin
//     serves makes the float action refuse the plan (mf_f32_build in zzz_matfree.hip; tools/mf_f32_host.cpp runs the same
//     decision on the CPU).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "element_tables.inc"

#if !defined(ZZZ_HD)
#if defined(__HIPCC__)
#define ZZZ_HD __host__ __device__
#else
#define ZZZ_HD
#endif
#endif

// Float on the device: an empty asm statement that takes the table offset together with the values just formed makes the
// next phase's table reads depend on this phase's results, so the scheduler cannot hoist them all to the top (it filled
// every register the launch bound allows with hoisted reads and the allocator then spilled)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZZZ_MF_YE4(i) "+v"(ye[i]), "+v"(ye[i + 1]), "+v"(ye[i + 2]), "+v"(ye[i + 3])
#define ZZZ_MF_FENCE_G() asm volatile("" : "+v"(off), "+v"(g[0]), "+v"(g[1]), "+v"(g[2]))
#define ZZZ_MF_FENCE_Y()                                                                                                \
  do                                                                                                                    \
  {                                                                                                                     \
    if constexpr (ND == 20)                                                                                             \
      asm volatile("" : "+v"(off), ZZZ_MF_YE4(0), ZZZ_MF_YE4(4), ZZZ_MF_YE4(8), ZZZ_MF_YE4(12), ZZZ_MF_YE4(16));         \
    else                                                                                                                \
      asm volatile("" : "+v"(off), ZZZ_MF_YE4(0), ZZZ_MF_YE4(4), "+v"(ye[ND - 2]), "+v"(ye[ND - 1]));                    \
  } while (0)
#else
#define ZZZ_MF_FENCE_G() ((void)0)
#define ZZZ_MF_FENCE_Y() ((void)0)
#endif
// where the statement stands: 1 after every mode, 2 (default) also between a mode's two phases -- 118 against 92 registers at
// P3, 4 against 5 wavefronts per SIMD; a build-time switch for A/B runs (-DZZZ_MF_FENCE_MODE=1)
#ifndef ZZZ_MF_FENCE_MODE
#define ZZZ_MF_FENCE_MODE 2
#endif

namespace zzz
{
template <typename R>
ZZZ_HD inline R mf_round(double v)
{
  return (R)v;
}
template <typename R>
ZZZ_HD inline R mf_rel_coord(double x, double origin)
{
  return (R)(x - origin);
}

// The factorised tables: constexpr copies decide at compile time which entries are zero; the values are staged in LDS
// by every (persistent) workgroup and reach the multiply-adds as broadcast reads.  (As literals they occupied ~200
// vector registers of every lane; as scalar loads from constant memory the compiler hoisted them all and spilled 865
// scalar registers; with the loads chained section by section through empty asm statements -- rows of the table as
// scalar operands, no LDS traffic for them -- the kernel still spilled 410 scalar registers into vector lanes and was
// 3 % faster at P3 6.2 M dofs, 0.281 against 0.291 ms, 1 % at P2: measured in round 4, not kept.)
template <int ND>
struct MfTab;
template <>
struct MfTab<10>
{
  static constexpr int NQ = 4;
  static constexpr bool nz(int a, int q, int j) { return ZZZ_DTAB_P2[(a * 4 + q) * 10 + j] != 0.0; }
};
template <>
struct MfTab<20>
{
  static constexpr int NQ = 10;
  static constexpr bool nz(int a, int q, int j) { return ZZZ_DTAB_P3[(a * 10 + q) * 20 + j] != 0.0; }
};

// y_e = sum_q sum_a D_a[q][:]^T h_a(q),  h(q) = G g(q),  g_a(q) = D_a[q][:] . u_e -- mode q by mode q, so that only u_e,
// y_e and six scalars are live.  A table entry is READ TWICE, once for each of its uses, the second time from a second
// copy of the table laid out for that use ([q][j][a]; the compiler cannot tell that the two are equal): kept in
// registers between the uses, the ~39 entries of a mode cost 78 vector registers, 220 in all, two wavefronts per SIMD.  Multiply-adds are fused here (the library is otherwise built with
// -ffp-contract=off): the action is compared with the oracle to a tolerance, not bit for bit.
template <int ND, typename R>
ZZZ_HD inline void mf_element_pk(const R* __restrict__ tab, const R* __restrict__ tabT, const R (&ue)[ND], const R (&G)[6],
                                 R (&ye)[ND])
{
#pragma clang fp contract(fast)
  constexpr int NQ = MfTab<ND>::NQ;
  [[maybe_unused]] int off = 0; // (always 0: see ZZZ_MF_FENCE_G / _Y above)
#pragma unroll
  for (int j = 0; j < ND; ++j)
    ye[j] = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    R g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      R acc = 0.0;
#pragma unroll
      for (int j = 0; j < ND; ++j)
        if (MfTab<ND>::nz(a, q, j))
          acc += (sizeof(R) == 4 ? tab[off + (a * NQ + q) * ND + j] : tab[(a * NQ + q) * ND + j]) * ue[j];
      g[a] = acc;
    }
    if constexpr (sizeof(R) == 4 && ZZZ_MF_FENCE_MODE >= 2)
      ZZZ_MF_FENCE_G();
    const R h0 = G[0] * g[0] + G[3] * g[1] + G[4] * g[2];
    const R h1 = G[3] * g[0] + G[1] * g[1] + G[5] * g[2];
    const R h2 = G[4] * g[0] + G[5] * g[1] + G[2] * g[2];
#pragma unroll
    for (int j = 0; j < ND; ++j)
    {
      if (MfTab<ND>::nz(0, q, j))
        ye[j] += (sizeof(R) == 4 ? tabT[off + (q * ND + j) * 3 + 0] : tabT[(q * ND + j) * 3 + 0]) * h0;
      if (MfTab<ND>::nz(1, q, j))
        ye[j] += (sizeof(R) == 4 ? tabT[off + (q * ND + j) * 3 + 1] : tabT[(q * ND + j) * 3 + 1]) * h1;
      if (MfTab<ND>::nz(2, q, j))
        ye[j] += (sizeof(R) == 4 ? tabT[off + (q * ND + j) * 3 + 2] : tabT[(q * ND + j) * 3 + 2]) * h2;
    }
    if constexpr (sizeof(R) == 4 && ZZZ_MF_FENCE_MODE >= 1)
      ZZZ_MF_FENCE_Y();
  }
}

// P2/P3: G = |detJ| K K^T of one cell from its four vertices, in double (the float action reads it rounded: mf_round);
// G = {G00, G11, G22, G01, G02, G12}
ZZZ_HD inline void mf_cell_geom(const double (&p)[4][3], double (&G)[6])
{
  double J[3][3];
  for (int a = 0; a < 3; ++a)
    for (int al = 0; al < 3; ++al)
      J[a][al] = p[al + 1][a] - p[0][a];
  // K = J^-1 = C / det, K[al][a] = dX_al / dx_a
  double C[3][3];
  C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  C[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
  C[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  C[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  C[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
  C[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  C[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
  C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  const double det = J[0][0] * C[0][0] + J[0][1] * C[1][0] + J[0][2] * C[2][0];
  const double sc = 1.0 / std::fabs(det); // |det| K K^T = C C^T / |det|
  const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
  for (int t = 0; t < 6; ++t)
    G[t] = (C[pa[t]][0] * C[pb[t]][0] + C[pa[t]][1] * C[pb[t]][1] + C[pa[t]][2] * C[pb[t]][2]) * sc;
}

// P1: p_k = {x, y, z, u} of vertex k.  J[a][al] = p_(al+1)[a] - p_0[a]; C = cofactors: K = J^-1 = C / det,
// grad phi_(al+1) = C[al][:] / det;  y_e = c (c^T u) / (6 |det J|).  DIAG: the element matrix's diagonal instead.
template <typename R>
struct MfPoint
{
  R x, y, z, w;
};
template <bool DIAG, typename R>
ZZZ_HD inline void mf_element_p1(const MfPoint<R>& p0, const MfPoint<R>& p1, const MfPoint<R>& p2, const MfPoint<R>& p3, R (&ye)[4])
{
#pragma clang fp contract(fast)
  const R J00 = p1.x - p0.x, J01 = p2.x - p0.x, J02 = p3.x - p0.x;
  const R J10 = p1.y - p0.y, J11 = p2.y - p0.y, J12 = p3.y - p0.y;
  const R J20 = p1.z - p0.z, J21 = p2.z - p0.z, J22 = p3.z - p0.z;
  const R C00 = J11 * J22 - J12 * J21, C01 = J02 * J21 - J01 * J22, C02 = J01 * J12 - J02 * J11;
  const R C10 = J12 * J20 - J10 * J22, C11 = J00 * J22 - J02 * J20, C12 = J02 * J10 - J00 * J12;
  const R C20 = J10 * J21 - J11 * J20, C21 = J01 * J20 - J00 * J21, C22 = J00 * J11 - J01 * J10;
  const R det = J00 * C00 + J01 * C10 + J02 * C20;
  const R d1 = p1.w - p0.w, d2 = p2.w - p0.w, d3 = p3.w - p0.w;
  const R sc = (R)1.0 / ((R)6.0 * std::fabs(det));
  if constexpr (DIAG)
  {
    const R s0 = C00 + C10 + C20, s1 = C01 + C11 + C21, s2 = C02 + C12 + C22;
    ye[0] = (s0 * s0 + s1 * s1 + s2 * s2) * sc;
    ye[1] = (C00 * C00 + C01 * C01 + C02 * C02) * sc;
    ye[2] = (C10 * C10 + C11 * C11 + C12 * C12) * sc;
    ye[3] = (C20 * C20 + C21 * C21 + C22 * C22) * sc;
  }
  else
  {
    const R t0 = (C00 * d1 + C10 * d2 + C20 * d3) * sc;
    const R t1 = (C01 * d1 + C11 * d2 + C21 * d3) * sc;
    const R t2 = (C02 * d1 + C12 * d2 + C22 * d3) * sc;
    ye[1] = C00 * t0 + C01 * t1 + C02 * t2;
    ye[2] = C10 * t0 + C11 * t1 + C12 * t2;
    ye[3] = C20 * t0 + C21 * t1 + C22 * t2;
    ye[0] = -(ye[1] + ye[2] + ye[3]);
  }
}

// ---- block size 3: form a of src/Elasticity.py, inner(sigma(u), eps(v)) dx, per cell, never stored -------------------------
// sigma = mu (H + H^T) + lambda tr(H) I with H the physical gradient of u; since sigma is symmetric, inner(sigma, eps(v)) =
// inner(sigma, grad v).  Double only (the float path keeps its block-size-3 refusal).
constexpr double MF_EL_E = 1.0e6, MF_EL_NU = 0.3; // src/Elasticity.py:12-15
constexpr double MF_EL_MU = MF_EL_E / (2.0 * (1.0 + MF_EL_NU));
constexpr double MF_EL_LAMBDA = MF_EL_E * MF_EL_NU / ((1.0 + MF_EL_NU) * (1.0 - 2.0 * MF_EL_NU));

// sg = mu (H + H^T) + lambda tr(H) I
ZZZ_HD inline void mf_el_sigma(const double (&H)[3][3], double (&sg)[3][3])
{
#pragma clang fp contract(fast)
  const double lt = MF_EL_LAMBDA * (H[0][0] + H[1][1] + H[2][2]);
  for (int c = 0; c < 3; ++c)
    for (int d = 0; d < 3; ++d)
      sg[c][d] = MF_EL_MU * (H[c][d] + H[d][c]) + (c == d ? lt : 0.0);
}

// P2/P3 geometry record: K = J^-1 (K[al][d] = dX_al / dx_d at Kd[3 al + d]) and |det J| at Kd[9], in double as mf_cell_geom
ZZZ_HD inline void mf_cell_geom_el(const double (&p)[4][3], double (&Kd)[10])
{
  double J[3][3];
  for (int a = 0; a < 3; ++a)
    for (int al = 0; al < 3; ++al)
      J[a][al] = p[al + 1][a] - p[0][a];
  double C[3][3];
  C[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  C[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
  C[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  C[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  C[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  C[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
  C[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  C[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
  C[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  const double det = J[0][0] * C[0][0] + J[0][1] * C[1][0] + J[0][2] * C[2][0];
  const double inv = 1.0 / det;
  for (int al = 0; al < 3; ++al)
    for (int d = 0; d < 3; ++d)
      Kd[3 * al + d] = C[al][d] * inv;
  Kd[9] = std::fabs(det);
}

// The factorised element of block size 3 in three phases, so that the caller never holds u_e and y_e of the three components
// at once (2 x 60 doubles at P3): with S^ab_ij = sum_q D_a[q][i] D_b[q][j], for every mode q
//   1. g[q][a] = D_a[q][:] . u_e^c                      (mf_el_modes, one component c at a time: u_e^c alone is live)
//   2. H[c][d] = sum_a g[c][q][a] K[a][d];  sigma(H);  T[c][q][a] = |det J| sum_d sigma[c][d] K[a][d]   (mf_el_stress, in place)
//   3. y_e^c[j] = sum_q sum_a D_a[q][j] T[c][q][a]      (mf_el_accumulate, one component at a time)
template <int ND>
ZZZ_HD inline void mf_el_modes(const double* __restrict__ tab, const double (&ue)[ND], double (&g)[MfTab<ND>::NQ][3])
{
#pragma clang fp contract(fast)
  constexpr int NQ = MfTab<ND>::NQ;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < ND; ++j)
        if (MfTab<ND>::nz(a, q, j))
          acc += tab[(a * NQ + q) * ND + j] * ue[j];
      g[q][a] = acc;
    }
}
template <int NQ>
ZZZ_HD inline void mf_el_stress(const double (&Kd)[10], double (&g)[3][NQ][3])
{
#pragma clang fp contract(fast)
#pragma unroll
  for (int q = 0; q < NQ; ++q)
  {
    double H[3][3], sg[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int d = 0; d < 3; ++d)
        H[c][d] = g[c][q][0] * Kd[d] + g[c][q][1] * Kd[3 + d] + g[c][q][2] * Kd[6 + d];
    mf_el_sigma(H, sg);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < 3; ++a)
        g[c][q][a] = Kd[9] * (sg[c][0] * Kd[3 * a] + sg[c][1] * Kd[3 * a + 1] + sg[c][2] * Kd[3 * a + 2]);
  }
}
template <int ND>
ZZZ_HD inline void mf_el_accumulate(const double* __restrict__ tabT, const double (&t)[MfTab<ND>::NQ][3], double (&ye)[ND])
{
#pragma clang fp contract(fast)
  constexpr int NQ = MfTab<ND>::NQ;
#pragma unroll
  for (int j = 0; j < ND; ++j)
    ye[j] = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int j = 0; j < ND; ++j)
    {
      if (MfTab<ND>::nz(0, q, j))
        ye[j] += tabT[(q * ND + j) * 3 + 0] * t[q][0];
      if (MfTab<ND>::nz(1, q, j))
        ye[j] += tabT[(q * ND + j) * 3 + 1] * t[q][1];
      if (MfTab<ND>::nz(2, q, j))
        ye[j] += tabT[(q * ND + j) * 3 + 2] * t[q][2];
    }
}
// the element matrix's diagonal: for (j, c) sum_q d^T M^cc d, d_a = D_a[q][j],
// M^cc_ab = |det J| (mu (K K^T)_ab + (mu + lambda) K[a][c] K[b][c]):  with v = K^T d,  |det J| (mu |v|^2 + (mu + lambda) v_c^2)
template <int ND>
ZZZ_HD inline void mf_el_diag_pk(const double* __restrict__ tabT, const double (&Kd)[10], double (&ye)[3][ND])
{
#pragma clang fp contract(fast)
  constexpr int NQ = MfTab<ND>::NQ;
#pragma unroll
  for (int j = 0; j < ND; ++j)
  {
    double vv = 0.0, v2[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
      if (!(MfTab<ND>::nz(0, q, j) || MfTab<ND>::nz(1, q, j) || MfTab<ND>::nz(2, q, j)))
        continue;
      const double d0 = tabT[(q * ND + j) * 3 + 0], d1 = tabT[(q * ND + j) * 3 + 1], d2 = tabT[(q * ND + j) * 3 + 2];
#pragma unroll
      for (int x = 0; x < 3; ++x)
      {
        const double v = d0 * Kd[x] + d1 * Kd[3 + x] + d2 * Kd[6 + x];
        vv += v * v;
        v2[x] += v * v;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ye[c][j] = Kd[9] * (MF_EL_MU * vv + (MF_EL_MU + MF_EL_LAMBDA) * v2[c]);
  }
}

// P1 from the vertex coordinates x[k][:] and values u[k][c]: cofactors and one division; H is constant on the cell.
// With H' = (u_(al+1) - u_0) C (the gradient times det J) and sigma linear:  y^c_(al+1) = sum_d sigma(H')[c][d] C[al][d] / (6 |det J|),
// y^c_0 = -(their sum).  DIAG: (j, c) -> (mu |C_j|^2 + (mu + lambda) C_j[c]^2) / (6 |det J|), C_0 = -(C_1 + C_2 + C_3).
template <bool DIAG>
ZZZ_HD inline void mf_el_element_p1(const double (&x)[4][3], const double (&u)[4][3], double (&ye)[4][3])
{
#pragma clang fp contract(fast)
  const double J00 = x[1][0] - x[0][0], J01 = x[2][0] - x[0][0], J02 = x[3][0] - x[0][0];
  const double J10 = x[1][1] - x[0][1], J11 = x[2][1] - x[0][1], J12 = x[3][1] - x[0][1];
  const double J20 = x[1][2] - x[0][2], J21 = x[2][2] - x[0][2], J22 = x[3][2] - x[0][2];
  double C[4][3];
  C[1][0] = J11 * J22 - J12 * J21, C[1][1] = J02 * J21 - J01 * J22, C[1][2] = J01 * J12 - J02 * J11;
  C[2][0] = J12 * J20 - J10 * J22, C[2][1] = J00 * J22 - J02 * J20, C[2][2] = J02 * J10 - J00 * J12;
  C[3][0] = J10 * J21 - J11 * J20, C[3][1] = J01 * J20 - J00 * J21, C[3][2] = J00 * J11 - J01 * J10;
  const double det = J00 * C[1][0] + J01 * C[2][0] + J02 * C[3][0];
  const double sc = 1.0 / (6.0 * std::fabs(det));
  if constexpr (DIAG)
  {
#pragma unroll
    for (int d = 0; d < 3; ++d)
      C[0][d] = -(C[1][d] + C[2][d] + C[3][d]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      const double cc = C[k][0] * C[k][0] + C[k][1] * C[k][1] + C[k][2] * C[k][2];
#pragma unroll
      for (int c = 0; c < 3; ++c)
        ye[k][c] = (MF_EL_MU * cc + (MF_EL_MU + MF_EL_LAMBDA) * C[k][c] * C[k][c]) * sc;
    }
  }
  else
  {
    double H[3][3], sg[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
      const double d1 = u[1][c] - u[0][c], d2 = u[2][c] - u[0][c], d3 = u[3][c] - u[0][c];
#pragma unroll
      for (int d = 0; d < 3; ++d)
        H[c][d] = d1 * C[1][d] + d2 * C[2][d] + d3 * C[3][d];
    }
    mf_el_sigma(H, sg);
#pragma unroll
    for (int c = 0; c < 3; ++c)
    {
#pragma unroll
      for (int k = 1; k < 4; ++k)
        ye[k][c] = (sg[c][0] * C[k][0] + sg[c][1] * C[k][1] + sg[c][2] * C[k][2]) * sc;
      ye[0][c] = -(ye[1][c] + ye[2][c] + ye[3][c]);
    }
  }
}

// ---- the right-hand side on the same plan: form L of src/Poisson.py (inner(f, v) dx + inner(g, v) ds) and of
// src/Elasticity.py (inner(f, v) dx), per cell (k_mf_rhs of zzz_matfree.hip; tools/mf_rhs_host.cpp runs the same code on the
// CPU).  M is the reference mass table the row-gather kernels read (tab[9 ND^2 ...] of element_tables.inc, [i][j]), F the four
// reference facet tables behind it (tab[10 ND^2 ...], [lf][i][j], rows of dofs off the facet are zero).  The products are
// formed in asm_vector_pk's order -- sum over j first, then the geometry factor -- with the library's two roundings per
// multiply-add: a cell contributes the same bits here and there, only the order of the cells differs.
// f_at(j, o) = the coefficient at local dof j; o is the chain's offset (always 0), which a caller short of registers adds to the
// address it reads so that a pass's reads wait for the pass before.  The columns are taken ten at a time at P3, so that half of f_e and half a row of
// the table are in flight beside the twenty sums, not all of both (128 registers hold the element then); a row's sum is still
// formed column by column from the left.  On the device the rows are chained through an empty asm statement, as
// ZZZ_MF_FENCE_G chains the action's modes: without it the scheduler hoists the ND^2 table reads to the top -- 256 registers
// and scratch at P2 already.
#if defined(__HIP_DEVICE_COMPILE__)
#define ZZZ_MF_RHS_FENCE(v) asm volatile("" : "+v"(off), "+v"(v))
#define ZZZ_MF_RHS_OPAQUE(o) asm volatile("" : "+v"(o))
#else
#define ZZZ_MF_RHS_FENCE(v) ((void)0)
#define ZZZ_MF_RHS_OPAQUE(o) ((void)0)
#endif
template <int ND, int NH = (ND == 20 ? 10 : ND), class FAt> // NH: columns per pass (k_mf_rhs: five at P3 with 1024 threads)
ZZZ_HD inline void mf_rhs_mass(const double* __restrict__ M, double adet, FAt&& f_at, double (&ye)[ND])
{
  static_assert(ND % NH == 0, "whole passes");
  [[maybe_unused]] int off = 0;          // (always 0)
#pragma unroll
  for (int j0 = 0; j0 < ND; j0 += NH)
  {
    double fe[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j)
      fe[j] = f_at(j0 + j, off);
#pragma unroll
    for (int i = 0; i < ND; ++i)
    {
      double acc = j0 == 0 ? 0.0 : ye[i];
#pragma unroll
      for (int j = 0; j < NH; ++j)
        acc += M[off + i * ND + j0 + j] * fe[j];
      ye[i] = j0 + NH == ND ? adet * acc : acc;
      ZZZ_MF_RHS_FENCE(ye[i]);
    }
  }
}
// block size 3: the same table per component, three values per node; f_at(j, c) = component c of the coefficient at local
// node j (and the chain's offset), one component at a time
template <int ND, class FAt>
ZZZ_HD inline void mf_rhs_mass3(const double* __restrict__ M, double adet, FAt&& f_at, double (&ye)[3][ND])
{
#pragma unroll
  for (int c = 0; c < 3; ++c)
    mf_rhs_mass<ND>(M, adet, [&](int j, int o) -> double { return f_at(j, c, o); }, ye[c]);
}
// exterior facet lf of a cell: y_e += scale * F[lf] g_e, scale = twice the facet's area; g_at(j) = the boundary coefficient
// at local dof j, fetched where it is used (the cells that have such a facet are a surface's worth)
template <int ND, class GAt>
ZZZ_HD inline void mf_rhs_facet(const double* __restrict__ F, int lf, double scale, GAt&& g_at, double (&ye)[ND])
{
  // (a loop over j per row, not unrolled, the row's offset formed where it is used: a handful of registers beside y_e)
#pragma unroll
  for (int i = 0; i < ND; ++i)
  {
    int o = (lf * ND + i) * ND;
    if constexpr (ND > 4) // (as a compile-time offset from a uniform base the ND row pointers are hoisted: 49 spilled SGPRs at P3)
      ZZZ_MF_RHS_OPAQUE(o);
    double fa = 0.0;
#pragma unroll 1
    for (int j = 0; j < ND; ++j)
      fa += F[o + j] * g_at(j);
    ye[i] += scale * fa;
  }
}

// ---- P1 in float: how well an origin serves a cell, which origin a block takes, or none ----------------------------------
// Column by column (column al = edge p_(al+1) - p_0), every entry of the Jacobian formed in float from the rounded relative
// coordinates is compared with the double Jacobian's, against the cell's extent along that entry's axis (per axis: an
// anisotropic or sheared cell is judged by what each coordinate has to resolve, as tests/_hp_ref.py judges the result against
// what its terms weigh): jerr, at most 2^-24 x (distance from the origin) / extent.  What real plans cost, any origin: a
// uniform mesh up to 32 units of 2^-24 (a Morton run of 2048 cells spans up to ~32 cell widths), the unstructured spoke mesh
// with its cells of aspect 31 65 .. 340 units; a mesh graded to a corner with the origin at the wrong end 10^4 .. 10^6.
//   * MF_F32_JKEEP (256 units): the block's first listed dof stays the origin while every cell is within it -- the plans
//     served before keep their bits;
//   * beyond it the better of the first and the second origin (MfF32Thin) is taken;
//   * MF_F32_JTOL (4096 units: the geometry keeps 12 of float's 24 bits) is where the float action refuses the block -- a
//     factor 10 beyond any mesh seen served, a factor 10 short of the meshes that came back wrong.
// The float determinant must also be safely away from zero (2^-18 of the sum of its terms' magnitudes: the float evaluation
// of that sum is off by at most ~2^-22 of it), have the double determinant's sign, and leave 1 / (6 |det|) and the cofactors
// inside float's range: `ok`.
constexpr double MF_F32_JKEEP = 0x1p-16, MF_F32_JTOL = 0x1p-12;
constexpr double MF_F32_DET_MARGIN = 0x1p-18, MF_F32_DET_MIN = 0x1p-100, MF_F32_DET_MAX = 0x1p100;

struct MfF32Verdict
{
  bool ok;      // the determinant's conditions
  double jerr;  // largest |J_float - J_double| / (extent of the cell along that axis)
  double ratio; // largest (distance of the cell from the origin) / (extent of the cell) over the three axes
};
// what a block does with the verdicts of its two origins (ok: every cell's; jerr: the largest): 0 first, 1 second, 2 refuse
ZZZ_HD inline bool mf_f32_keep_first(bool ok0, double j0, double jtol) { return ok0 && j0 <= (MF_F32_JKEEP < jtol ? MF_F32_JKEEP : jtol); }
ZZZ_HD inline int mf_f32_choose(bool ok0, double j0, bool ok1, double j1, double jtol)
{
  const bool c0 = ok0 && j0 <= jtol, c1 = ok1 && j1 <= jtol;
  return c1 && (!c0 || j1 < j0) ? 1 : (c0 ? 0 : 2);
}

// lowest coordinate and extent of a cell along every axis
ZZZ_HD inline void mf_f32_extent(const double (&p)[4][3], double (&lo)[3], double (&ext)[3])
{
  for (int a = 0; a < 3; ++a)
  {
    double l = p[0][a], h = p[0][a];
    for (int k = 1; k < 4; ++k)
    {
      l = p[k][a] < l ? p[k][a] : l;
      h = p[k][a] > h ? p[k][a] : h;
    }
    lo[a] = l;
    ext[a] = h - l;
  }
}

ZZZ_HD inline MfF32Verdict mf_f32_cell(const double (&p)[4][3], const double (&o)[3])
{
  double lo[3], ext[3], Jf[3][3], Jd[3][3];
  mf_f32_extent(p, lo, ext);
  MfF32Verdict v = {true, 0.0, 0.0};
  for (int a = 0; a < 3; ++a)
  {
    const float r0 = mf_rel_coord<float>(p[0][a], o[a]);
    double far = std::fabs(p[0][a] - o[a]);
    for (int al = 0; al < 3; ++al)
    {
      const float r = mf_rel_coord<float>(p[al + 1][a], o[a]);
      Jf[a][al] = (double)(r - r0); // (the float subtraction of mf_element_p1)
      Jd[a][al] = p[al + 1][a] - p[0][a];
      far = std::fmax(far, std::fabs(p[al + 1][a] - o[a]));
      if (ext[a] > 0.0)
        v.jerr = std::fmax(v.jerr, std::fabs(Jf[a][al] - Jd[a][al]) / ext[a]);
    }
    if (!(ext[a] > 0.0))
    {
      v.ok = false;
      v.jerr = HUGE_VAL;
    }
    v.ratio = std::fmax(v.ratio, ext[a] > 0.0 ? far / ext[a] : HUGE_VAL);
  }
  // the determinant of the FLOAT Jacobian, its terms as mf_element_p1 groups them
  double det = 0.0, mag = 0.0, detd = 0.0;
  for (int al = 0; al < 3; ++al)
  {
    const int b = (al + 1) % 3, c = (al + 2) % 3;
    det += Jf[0][al] * (Jf[1][b] * Jf[2][c] - Jf[1][c] * Jf[2][b]);
    mag += std::fabs(Jf[0][al]) * (std::fabs(Jf[1][b] * Jf[2][c]) + std::fabs(Jf[1][c] * Jf[2][b]));
    detd += Jd[0][al] * (Jd[1][b] * Jd[2][c] - Jd[1][c] * Jd[2][b]);
  }
  if (!(std::fabs(det) >= MF_F32_DET_MARGIN * mag) || !(std::fabs(det) >= MF_F32_DET_MIN) || !(std::fabs(det) <= MF_F32_DET_MAX)
      || (det > 0.0) != (detd > 0.0))
    v.ok = false;
  return v;
}

// The second origin, tried where the block's first listed dof is past MF_F32_JKEEP: axis by axis, stand where the block is
// finest -- the lowest coordinate among the cells whose extent along that axis is within a factor 2 of the block's least.
// Two passes over the block's cells (least extent, then lowest coordinate), both plain minima: the result does not depend
// on the order of the cells.  (The block's min corner serves a mesh graded towards low coordinates only; a mesh graded
// towards the far corner needs the origin there.)
struct MfF32Thin
{
  double ext[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, at[3] = {DBL_MAX, DBL_MAX, DBL_MAX};
};
ZZZ_HD inline void mf_f32_thin_ext(MfF32Thin& t, const double (&p)[4][3])
{
  double lo[3], ext[3];
  mf_f32_extent(p, lo, ext);
  for (int a = 0; a < 3; ++a)
    t.ext[a] = ext[a] < t.ext[a] ? ext[a] : t.ext[a];
}
ZZZ_HD inline void mf_f32_thin_at(MfF32Thin& t, const double (&p)[4][3])
{
  double lo[3], ext[3];
  mf_f32_extent(p, lo, ext);
  for (int a = 0; a < 3; ++a)
    if (ext[a] <= 2.0 * t.ext[a] && lo[a] < t.at[a])
      t.at[a] = lo[a];
}
} // namespace zzz
