// ZZZ_PC_PMG: the transfer between the Pk (k = 2, 3) and the P1 space on ONE generated cube -- the level pair that
// zzz_mg.hip puts in front of its P1 hierarchy.  No P is stored, nothing is added atomically, every sum has one order.
//
// Every Pk dof of the Kuhn cube (host/cube_layout.h) sits on an entity anchored at its lowest lattice point a, and the P1
// function evaluated there has at most three terms:
//   vertex                         1 on a
//   edge, axis mask m, sub-dof s   (1 - t_s) on a, t_s on a + m;  t = make_cell's tt (0.5 at P2, the GLL points at P3)
//   face (S1, S2)                  1/3 on each of a, a + S1, a + S1 + S2
// An entity exists when a + (its mask) stays inside the lattice.  The fine dofs are numbered by zzzcube::Layout, whose
// vertex / edge / face give every index here; the P1 dofs are the lattice points in lexicographic order.
// P~ = F_k P F_1 with F zeroing the constrained dofs; block size 3 per component.
//
// Both kernels run one thread per lattice point and component (the components of a dof are adjacent in memory, so
// neighbouring lanes still touch neighbouring entries).  The masks are the constants of fully unrolled loops, so Layout's
// switches fold and no index lives in an indexed private array (no scratch).
#pragma once
#include "../host/cube_layout.h"

namespace zzz
{
using zzzcube::Layout;

// the twelve faces anchored at a lattice point: two each in the xy, xz and yz planes, six inside the sub-cube
#define PMG_FACES(F) F(1, 2) F(2, 1) F(1, 4) F(4, 1) F(2, 4) F(4, 2) F(1, 6) F(2, 5) F(4, 3) F(6, 1) F(5, 2) F(3, 4)

template <int ORDER>
struct PmgT
{
  // (1 - 1/sqrt5)/2 and (1 + 1/sqrt5)/2 as make_cell forms them
  static ZZZ_HD inline double t(int s)
  {
    const double sq5 = 2.23606797749978969640917366873128;
    return ORDER == 2 ? 0.5 : (s == 0 ? 0.5 * (1.0 - 1.0 / sq5) : 0.5 * (1.0 + 1.0 / sq5));
  }
};

// a + mask stays inside the lattice (a itself is inside)
template <int M>
ZZZ_HD inline bool pmg_room(const Layout& L, int64_t ix, int64_t iy, int64_t iz)
{
  return (!(M & 1) || ix < L.nx) && (!(M & 2) || iy < L.ny) && (!(M & 4) || iz < L.nz);
}
// a - mask stays inside the lattice
template <int M>
ZZZ_HD inline bool pmg_back(int64_t ix, int64_t iy, int64_t iz)
{
  return (!(M & 1) || ix > 0) && (!(M & 2) || iy > 0) && (!(M & 4) || iz > 0);
}

// x_k (+)= P~ e_1, entry u = (lattice point, component): the eight corners of the sub-cube anchored at the point are gathered
// once; every store of a wavefront goes to consecutive entities of one type block
template <int ORDER, int BS>
ZZZ_HD inline void pmg_prolong_entry(const Layout& L, int64_t u, const uint8_t* __restrict__ bcf, const uint8_t* __restrict__ bcc,
                                     const double* __restrict__ ec, double* __restrict__ xf, int accumulate)
{
  constexpr int NPE = ORDER - 1;
  const int64_t v = u / BS;
  const int k = (int)(u % BS);
  const int64_t ix = v % L.PX, iy = (v / L.PX) % L.PY, iz = v / (L.PX * L.PY);
  const int64_t a[3] = {ix, iy, iz};
  auto put = [&](int64_t dof, double s) {
    const int64_t i = dof * BS + k;
    if (bcf[i])
      s = 0.0;
    xf[i] = accumulate ? xf[i] + s : s;
  };
  // corner d of the sub-cube: the lattice point a + d, zero when outside or constrained
  double e[8];
#pragma unroll
  for (int d = 0; d < 8; ++d)
  {
    const bool in = (!(d & 1) || ix < L.nx) && (!(d & 2) || iy < L.ny) && (!(d & 4) || iz < L.nz);
    const int64_t j = (v + (d & 1 ? 1 : 0) + (d & 2 ? L.PX : 0) + (d & 4 ? L.PX * L.PY : 0)) * BS + k;
    e[d] = in ? (bcc[j] ? 0.0 : ec[j]) : 0.0;
  }
  put(L.vertex(a), e[0]);
#pragma unroll
  for (int m = 1; m < 8; ++m)
  {
    const bool in = (!(m & 1) || ix < L.nx) && (!(m & 2) || iy < L.ny) && (!(m & 4) || iz < L.nz);
    if (in)
    {
#pragma unroll
      for (int s = 0; s < NPE; ++s)
      {
        const double t = PmgT<ORDER>::t(s);
        put(L.edge(a, m, s), (1.0 - t) * e[0] + t * e[m]);
      }
    }
  }
  if (ORDER == 3)
  {
    const double w = 1.0 / 3.0;
#define PMG_F(S1, S2)                                                                                                 \
  if (pmg_room<(S1) | (S2)>(L, ix, iy, iz))                                                                           \
    put(L.face(a, S1, S2), w * e[0] + w * e[S1] + w * e[(S1) | (S2)]);
    PMG_FACES(PMG_F)
#undef PMG_F
  }
}

// r_1 = P~^T (r_k - sub) in gather form, entry u = (lattice point, component): the thread reads its vertex dof, per mask the edge
// anchored at the point and the edge ending there, and the faces that have the point as first, second or third vertex -- at
// most 1 + 14 (k - 1) + 36 [k = 3] reads, in this order in every run.  The bounds come from the lattice.
template <int ORDER, int BS>
ZZZ_HD inline void pmg_restrict_entry(const Layout& L, int64_t u, const uint8_t* __restrict__ bcf, const uint8_t* __restrict__ bcc,
                                      const double* __restrict__ rf, const double* __restrict__ sub, double* __restrict__ rc)
{
  constexpr int NPE = ORDER - 1;
  const int64_t v = u / BS;
  const int k = (int)(u % BS);
  const int64_t ix = v % L.PX, iy = (v / L.PX) % L.PY, iz = v / (L.PX * L.PY);
  const int64_t a[3] = {ix, iy, iz};
  auto get = [&](int64_t dof) -> double {
    const int64_t i = dof * BS + k;
    const double r = sub ? rf[i] - sub[i] : rf[i];
    return bcf[i] ? 0.0 : r;
  };
  double acc = get(L.vertex(a));
#pragma unroll
  for (int m = 1; m < 8; ++m)
  {
    const bool fwd = (!(m & 1) || ix < L.nx) && (!(m & 2) || iy < L.ny) && (!(m & 4) || iz < L.nz);
    const bool bwd = (!(m & 1) || ix > 0) && (!(m & 2) || iy > 0) && (!(m & 4) || iz > 0);
    const int64_t p[3] = {ix - (m & 1 ? 1 : 0), iy - (m & 2 ? 1 : 0), iz - (m & 4 ? 1 : 0)};
#pragma unroll
    for (int s = 0; s < NPE; ++s)
    {
      const double t = PmgT<ORDER>::t(s);
      if (fwd)
        acc += (1.0 - t) * get(L.edge(a, m, s));
      if (bwd)
        acc += t * get(L.edge(p, m, s));
    }
  }
  if (ORDER == 3)
  {
    const double w = 1.0 / 3.0;
    // first vertex: anchored here; second: anchored at a - S1 (and a + S2 inside); third: anchored at a - S1 - S2
#define PMG_F(S1, S2)                                                                                                 \
  {                                                                                                                   \
    if (pmg_room<(S1) | (S2)>(L, ix, iy, iz))                                                                         \
      acc += w * get(L.face(a, S1, S2));                                                                              \
    if (pmg_back<S1>(ix, iy, iz) && pmg_room<S2>(L, ix, iy, iz))                                                      \
    {                                                                                                                 \
      const int64_t p[3] = {ix - ((S1) & 1 ? 1 : 0), iy - ((S1) & 2 ? 1 : 0), iz - ((S1) & 4 ? 1 : 0)};               \
      acc += w * get(L.face(p, S1, S2));                                                                              \
    }                                                                                                                 \
    if (pmg_back<(S1) | (S2)>(ix, iy, iz))                                                                            \
    {                                                                                                                 \
      const int64_t p[3] = {ix - (((S1) | (S2)) & 1 ? 1 : 0), iy - (((S1) | (S2)) & 2 ? 1 : 0),                       \
                            iz - (((S1) | (S2)) & 4 ? 1 : 0)};                                                        \
      acc += w * get(L.face(p, S1, S2));                                                                              \
    }                                                                                                                 \
  }
    PMG_FACES(PMG_F)
#undef PMG_F
  }
  rc[u] = bcc[u] ? 0.0 : acc;
}
} // namespace zzz
