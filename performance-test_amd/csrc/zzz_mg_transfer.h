// The grid transfer of ZZZ_PC_MG (zzz_mg.hip): what its two kernels, its host code and a stand-alone host program
// (tools/mg_slab_host.cpp, under the sanitizers) share.  Host-compilable, as zzz_sagg_rows.h is.
//   * MgGeom: one level pair -- vertices per axis, where an axis starts in the tables, and the WINDOW of fine vertex planes
//     [z0, z1] whose vectors the caller holds: the whole cube is the window [0, nz]; a z-slab of host/cube_layout.h holds the
//     planes it owns, contiguous and in the cube's order, so a fine vector is indexed ((iz - z0) py + iy) px + ix.  The coarse
//     vectors are whole on either side; [cz0, cz1] are the coarse planes that the window's simplices can reach;
//   * mg_fill_tables: the three small tables per axis, in integers on the host;
//   * mg_simplex: the Kuhn simplex of the coarse cube that holds a fine vertex;
//   * mg_prolong_vertex, mg_restrict_vertex: the two walks, one fine vertex / one coarse vertex each.
#pragma once
#include <cstdint>

#if !defined(ZZZ_HD)
#if defined(__HIPCC__)
#define ZZZ_HD __host__ __device__
#else
#define ZZZ_HD
#endif
#endif

namespace zzz
{
// one level pair: vertices per axis, table offsets of the axes (fine tables: c and f per fine index; coarse tables: the
// range of fine indices whose simplex can touch a coarse index)
struct MgGeom
{
  int32_t pf[3], pc[3]; // vertices per axis, fine / coarse: of the whole cube
  int32_t of[3], oc[3]; // where axis a starts in the fine / coarse tables
  int32_t bs;
  int32_t z0, z1;   // the window of fine vertex planes (the whole cube: 0, pf[2] - 1)
  int32_t cz0, cz1; // the coarse vertex planes that planes [z0, z1] reach (the whole cube: 0, pc[2] - 1)
  int64_t nfv, ncv; // fine vertices of the window, coarse vertices of planes [cz0, cz1]
};

struct MgSimplex
{
  int32_t j[4]; // coarse vertices
  double w[4];
};

// The tables of a level pair of nf / nc cells per axis and the window [z0, z1] of fine planes: tc, tf of sum(nf + 1) entries
// (c_a = min(i nc / nf, nc - 1) and f_a = double(i nc - c_a nf) / double(nf) in 64-bit integers), rng of 2 sum(nc + 1) (first
// and last fine index whose simplex can reach a coarse index).  The caller sizes them: mg_table_sizes.
inline void mg_table_sizes(const int64_t nf[3], const int64_t nc[3], int64_t* nf_tot, int64_t* nc_tot)
{
  *nf_tot = nf[0] + nf[1] + nf[2] + 3;
  *nc_tot = nc[0] + nc[1] + nc[2] + 3;
}
inline void mg_fill_tables(MgGeom& G, const int64_t nf[3], const int64_t nc[3], int bs, int64_t z0, int64_t z1, int32_t* tc,
                           double* tf, int32_t* rng)
{
  G.bs = bs;
  int32_t nf_tot = 0, nc_tot = 0;
  for (int a = 0; a < 3; ++a)
  {
    G.pf[a] = (int32_t)nf[a] + 1;
    G.pc[a] = (int32_t)nc[a] + 1;
    G.of[a] = nf_tot;
    G.oc[a] = nc_tot;
    nf_tot += G.pf[a];
    nc_tot += G.pc[a];
  }
  for (int a = 0; a < 3; ++a)
  {
    const int64_t f = nf[a], c = nc[a];
    for (int64_t j = 0; j <= c; ++j)
    {
      rng[2 * (G.oc[a] + j)] = INT32_MAX;
      rng[2 * (G.oc[a] + j) + 1] = -1;
    }
    for (int64_t i = 0; i <= f; ++i)
    {
      const int64_t ci = i * c / f < c - 1 ? i * c / f : c - 1;
      tc[G.of[a] + i] = (int32_t)ci;
      tf[G.of[a] + i] = (double)(i * c - ci * f) / (double)f;
      // fine index i can reach coarse indices ci and ci + 1 of this axis
      for (int64_t j = ci; j <= ci + 1; ++j)
      {
        int32_t* r = &rng[2 * (G.oc[a] + j)];
        r[0] = r[0] < (int32_t)i ? r[0] : (int32_t)i;
        r[1] = r[1] > (int32_t)i ? r[1] : (int32_t)i;
      }
    }
  }
  G.z0 = (int32_t)z0;
  G.z1 = (int32_t)z1;
  G.cz0 = tc[G.of[2] + z0];
  G.cz1 = tc[G.of[2] + z1] + 1; // (c <= nc - 1: inside the cube)
  G.nfv = (int64_t)G.pf[0] * G.pf[1] * (z1 - z0 + 1);
  G.ncv = (int64_t)G.pc[0] * G.pc[1] * (G.cz1 - G.cz0 + 1);
}

// fine vertex (ix, iy, iz), iz counted in the whole cube
// (values and axes travel through the three compare-exchanges in registers: no indexed private array, no scratch)
ZZZ_HD inline MgSimplex mg_simplex(const MgGeom& G, const int32_t* __restrict__ tc, const double* __restrict__ tf, int ix, int iy,
                                   int iz)
{
  const int cx = tc[G.of[0] + ix], cy = tc[G.of[1] + iy], cz = tc[G.of[2] + iz];
  double v0 = tf[G.of[0] + ix], v1 = tf[G.of[1] + iy], v2 = tf[G.of[2] + iz];
  const int sx = 1, sy = G.pc[0], sz = G.pc[0] * G.pc[1];
  int s0 = sx, s1 = sy, s2 = sz;
  // descending, ties to the lower axis: strict comparisons of neighbours keep equal values in axis order
  if (v1 > v0)
  {
    const double t = v0; v0 = v1; v1 = t;
    const int u = s0; s0 = s1; s1 = u;
  }
  if (v2 > v1)
  {
    const double t = v1; v1 = v2; v2 = t;
    const int u = s1; s1 = s2; s2 = u;
  }
  if (v1 > v0)
  {
    const double t = v0; v0 = v1; v1 = t;
    const int u = s0; s0 = s1; s1 = u;
  }
  MgSimplex S;
  S.j[0] = (cz * G.pc[1] + cy) * G.pc[0] + cx;
  S.j[1] = S.j[0] + s0;
  S.j[2] = S.j[1] + s1;
  S.j[3] = S.j[2] + s2;
  S.w[0] = 1.0 - v0;
  S.w[1] = v0 - v1;
  S.w[2] = v1 - v2;
  S.w[3] = v2;
  return S;
}

// x_f (+)= P~ e_c at fine vertex v of the window (v = (k py + iy) px + ix, plane z0 + k of the cube): four gathers per
// component from the whole coarse vector, summed in the simplex's order; bcf / xf are indexed as the window's vectors are
ZZZ_HD inline void mg_prolong_vertex(const MgGeom& G, const int32_t* __restrict__ tc, const double* __restrict__ tf,
                                     const uint8_t* __restrict__ bcf, const uint8_t* __restrict__ bcc, const double* __restrict__ ec,
                                     double* __restrict__ xf, int accumulate, int64_t v)
{
  const int ix = (int)(v % G.pf[0]), iy = (int)((v / G.pf[0]) % G.pf[1]), iz = G.z0 + (int)(v / ((int64_t)G.pf[0] * G.pf[1]));
  const MgSimplex S = mg_simplex(G, tc, tf, ix, iy, iz);
  for (int k = 0; k < G.bs; ++k)
  {
    const int64_t i = v * G.bs + k;
    double e[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q)
    {
      const int64_t j = (int64_t)S.j[q] * G.bs + k;
      e[q] = bcc[j] ? 0.0 : ec[j];
    }
    double s = S.w[0] * e[0];
    s += S.w[1] * e[1];
    s += S.w[2] * e[2];
    s += S.w[3] * e[3];
    if (bcf[i])
      s = 0.0;
    xf[i] = accumulate ? xf[i] + s : s;
  }
}

// r_c = P~^T r_f at coarse vertex c (of the whole cube) in gather form: the fine vertices OF THE WINDOW whose simplex can hold
// it, in ascending (i_z, i_y, i_x) -- no atomics, the same bits in every run.  sub != null: r_f = b - sub, the residual formed
// on the way in.  A window that is not the whole cube leaves a partial sum: the windows of a partition add up to the whole.
template <int BS>
ZZZ_HD inline void mg_restrict_vertex(const MgGeom& G, const int32_t* __restrict__ tc, const double* __restrict__ tf,
                                      const int32_t* __restrict__ rng, const uint8_t* __restrict__ bcf,
                                      const uint8_t* __restrict__ bcc, const double* __restrict__ rf, const double* __restrict__ sub,
                                      double* __restrict__ rc, int64_t c)
{
  const int Cx = (int)(c % G.pc[0]), Cy = (int)((c / G.pc[0]) % G.pc[1]), Cz = (int)(c / ((int64_t)G.pc[0] * G.pc[1]));
  const int x0 = rng[2 * (G.oc[0] + Cx)], x1 = rng[2 * (G.oc[0] + Cx) + 1];
  const int y0 = rng[2 * (G.oc[1] + Cy)], y1 = rng[2 * (G.oc[1] + Cy) + 1];
  int z0 = rng[2 * (G.oc[2] + Cz)], z1 = rng[2 * (G.oc[2] + Cz) + 1];
  z0 = z0 > G.z0 ? z0 : G.z0;
  z1 = z1 < G.z1 ? z1 : G.z1;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  for (int iz = z0; iz <= z1; ++iz)
    for (int iy = y0; iy <= y1; ++iy)
      for (int ix = x0; ix <= x1; ++ix)
      {
        const MgSimplex S = mg_simplex(G, tc, tf, ix, iy, iz);
        // the four vertices of a simplex are distinct: at most one of them is this thread's
        double w;
        if (S.j[0] == (int32_t)c)
          w = S.w[0];
        else if (S.j[1] == (int32_t)c)
          w = S.w[1];
        else if (S.j[2] == (int32_t)c)
          w = S.w[2];
        else if (S.j[3] == (int32_t)c)
          w = S.w[3];
        else
          continue;
        const int64_t i = (((int64_t)(iz - G.z0) * G.pf[1] + iy) * G.pf[0] + ix) * BS;
        {
          double v = sub ? rf[i] - sub[i] : rf[i];
          if (bcf[i])
            v = 0.0;
          acc0 += w * v;
        }
        if (BS == 3)
        {
          double v = sub ? rf[i + 1] - sub[i + 1] : rf[i + 1];
          if (bcf[i + 1])
            v = 0.0;
          acc1 += w * v;
          v = sub ? rf[i + 2] - sub[i + 2] : rf[i + 2];
          if (bcf[i + 2])
            v = 0.0;
          acc2 += w * v;
        }
      }
  const int64_t o = c * BS;
  rc[o] = bcc[o] ? 0.0 : acc0;
  if (BS == 3)
  {
    rc[o + 1] = bcc[o + 1] ? 0.0 : acc1;
    rc[o + 2] = bcc[o + 2] ? 0.0 : acc2;
  }
}

// the planes [p0, p1] of fine vertices that part `part` of `nparts` z-slabs of an nz-cell cube owns (host/cube_layout.h, order 1:
// Slab::zs, ze -- plane zs belongs to the part below)
inline void mg_slab_planes(int64_t nz, int nparts, int part, int64_t* p0, int64_t* p1)
{
  const int64_t zs = nz * part / nparts, ze = nz * (part + 1) / nparts;
  *p0 = part == 0 ? 0 : zs + 1;
  *p1 = ze;
}
} // namespace zzz
