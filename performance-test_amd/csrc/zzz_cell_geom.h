// A cell's geometry as the assembly kernels form it: |det J| and J^-1 from the four vertices, the vertices of a facet and twice
// its area.  Shared by the row-gather kernels (zzz_asm_elem.h) and the cell-block right-hand side (k_mf_rhs of zzz_matfree.hip);
// host-compilable, so that tools/mf_rhs_host.cpp runs the same expressions on the CPU under the sanitizers.
#pragma once
#include <cmath>

#if !defined(ZZZ_HD)
#if defined(__HIPCC__)
#define ZZZ_HD __host__ __device__
#else
#define ZZZ_HD
#endif
#endif

namespace zzz
{
struct Geom
{
  double adet;    // |det J|
  double K[3][3]; // J^-1: K[al][a] = dX_al/dx_a
};

ZZZ_HD inline void geometry(const double p[4][3], Geom& G)
{
  double J[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int al = 0; al < 3; ++al)
      J[a][al] = p[al + 1][a] - p[0][a];
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][0] * J[2][2] - J[1][2] * J[2][0];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 - J[0][1] * c01 + J[0][2] * c02;
  const double id = 1.0 / det;
  G.adet = std::fabs(det);
  G.K[0][0] = c00 * id;
  G.K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
  G.K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
  G.K[1][0] = -c01 * id;
  G.K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
  G.K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
  G.K[2][0] = c02 * id;
  G.K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
  G.K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
}

// facet lf of a cell = the three vertices other than lf
ZZZ_HD inline void facet_vertices(int lf, int& q0, int& q1, int& q2)
{
  q0 = lf == 0 ? 1 : 0;
  q1 = lf <= 1 ? 2 : 1;
  q2 = lf == 3 ? 2 : 3;
}
// ... and twice its area, the scale of the exterior-facet terms
ZZZ_HD inline double facet_scale(const double p[4][3], int lf)
{
  int q0, q1, q2;
  facet_vertices(lf, q0, q1, q2);
  double e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    e1[k] = p[q1][k] - p[q0][k];
    e2[k] = p[q2][k] - p[q0][k];
  }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  return std::sqrt(cx * cx + cy * cy + cz * cz);
}
// ... of a facet given by its three vertices in the order of facet_vertices, for a caller that fetches those three alone: they
// stand as vertices 1, 2, 3 of a cell whose facet 0 they are, and facet_scale forms what it forms for the cell's own facet
ZZZ_HD inline double facet_scale_of(const double (&v)[3][3])
{
  const double p[4][3] = {{0.0, 0.0, 0.0}, {v[0][0], v[0][1], v[0][2]}, {v[1][0], v[1][1], v[1][2]}, {v[2][0], v[2][1], v[2][2]}};
  return facet_scale(p, 0);
}
} // namespace zzz
