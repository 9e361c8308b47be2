// The float action's per-cell code (csrc/zzz_mf_elem.h: rounding of the geometry factors and tables, block-relative P1
// coordinates, the element arithmetic the kernel's lanes run) on the CPU, for runs under the sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ../csrc mf_f32_host.cpp -o mf_f32_host
//   mf_f32_host IN OUT
//
// IN:  int32 order, ncells, ndofs, cells per block; double xc[ncells][4][3] (vertex coordinates of every cell);
//      int32 cell_dofs[ncells][nd]; double u[ndofs].
// OUT: float ye[ncells][nd], the element vectors.  tests/test_f32_host_program.py scatters them and compares the action
// with the numpy restatement's.  A block is `cells per block` consecutive cells; its origin is its first cell's first vertex.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zzz_mf_elem.h"

using namespace zzz;

template <int ND>
static void run_pk(const double* dtab, int nc, const std::vector<double>& xc, const std::vector<int32_t>& cd,
                   const std::vector<float>& u, std::vector<float>& out)
{
  constexpr int NQ = MfTab<ND>::NQ, NT = 3 * NQ * ND;
  std::vector<float> tab(NT), tabT(NT);
  for (int k = 0; k < NT; ++k) // the kernel's two layouts: [a][q][j] and [q][j][a]
  {
    const int a = k / (NQ * ND), q = (k / ND) % NQ, j = k % ND;
    tab[k] = mf_round<float>(dtab[k]);
    tabT[(q * ND + j) * 3 + a] = tab[k];
  }
  for (int c = 0; c < nc; ++c)
  {
    double p[4][3], G[6];
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a)
        p[k][a] = xc[(size_t)c * 12 + 3 * k + a];
    mf_cell_geom(p, G);
    float G32[6], ue[ND], ye[ND];
    for (int t = 0; t < 6; ++t)
      G32[t] = mf_round<float>(G[t]);
    for (int j = 0; j < ND; ++j)
      ue[j] = u[(size_t)cd[(size_t)c * ND + j]];
    mf_element_pk<ND, float>(tab.data(), tabT.data(), ue, G32, ye);
    for (int j = 0; j < ND; ++j)
      out[(size_t)c * ND + j] = ye[j];
  }
}

static void run_p1(int nc, int block, const std::vector<double>& xc, const std::vector<int32_t>& cd, const std::vector<float>& u,
                   std::vector<float>& out)
{
  for (int c = 0; c < nc; ++c)
  {
    const double* o = &xc[(size_t)(c / block) * block * 12]; // the block's origin
    MfPoint<float> p[4];
    for (int k = 0; k < 4; ++k)
    {
      const double* q = &xc[(size_t)c * 12 + 3 * k];
      p[k] = {mf_rel_coord<float>(q[0], o[0]), mf_rel_coord<float>(q[1], o[1]), mf_rel_coord<float>(q[2], o[2]),
              u[(size_t)cd[(size_t)c * 4 + k]]};
    }
    float ye[4];
    mf_element_p1<false, float>(p[0], p[1], p[2], p[3], ye);
    for (int j = 0; j < 4; ++j)
      out[(size_t)c * 4 + j] = ye[j];
  }
}

int main(int argc, char** argv)
{
  if (argc != 3)
    return std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  int32_t h[4];
  if (!f || std::fread(h, 4, 4, f) != 4)
    return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  const int order = h[0], nc = h[1], n = h[2], block = h[3];
  const int nd = order == 1 ? 4 : (order == 2 ? 10 : 20);
  if (order < 1 || order > 3 || nc < 1 || n < 1 || block < 1)
    return std::fprintf(stderr, "bad header\n"), 2;
  std::vector<double> xc((size_t)nc * 12), ud((size_t)n);
  std::vector<int32_t> cd((size_t)nc * nd);
  if (std::fread(xc.data(), 8, xc.size(), f) != xc.size() || std::fread(cd.data(), 4, cd.size(), f) != cd.size()
      || std::fread(ud.data(), 8, ud.size(), f) != ud.size())
    return std::fprintf(stderr, "short input\n"), 2;
  std::fclose(f);
  for (int32_t d : cd)
    if (d < 0 || d >= n)
      return std::fprintf(stderr, "dof out of range\n"), 2;
  std::vector<float> u((size_t)n), out((size_t)nc * nd);
  for (int i = 0; i < n; ++i)
    u[(size_t)i] = mf_round<float>(ud[(size_t)i]);
  if (order == 1)
    run_p1(nc, block, xc, cd, u, out);
  else if (order == 2)
    run_pk<10>(ZZZ_DTAB_P2, nc, xc, cd, u, out);
  else
    run_pk<20>(ZZZ_DTAB_P3, nc, xc, cd, u, out);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size())
    return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  std::fclose(f);
  return 0;
}
