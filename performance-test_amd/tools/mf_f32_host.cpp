// The float action's per-cell code (csrc/zzz_mf_elem.h: rounding of the geometry factors and tables, block-relative P1
// coordinates, the element arithmetic the kernel's lanes run) on the CPU, for runs under the sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-divide-by-zero -I ../csrc mf_f32_host.cpp -o mf_f32_host
//   mf_f32_host IN OUT [STATUS]
//
// IN:  int32 order, ncells, ndofs, cells per block; double xc[ncells][4][3] (vertex coordinates of every cell);
//      int32 cell_dofs[ncells][nd]; double u[ndofs].
// OUT: float ye[ncells][nd], the element vectors.  STATUS (P1, optional): int32 status[blocks].  tests/test_f32_host_program.py scatters
// them and compares the action with the numpy restatement's.  A block is `cells per block` consecutive cells (the caller
// orders them); its first origin is its first cell's first vertex, and what decides whether that origin serves the block,
// the second origin and the refusal are the library's own code (zzz_mf_elem.h).  A division by zero ends the run.
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

// P1 as mf_f32_build (csrc/zzz_matfree.hip) decides it: the block's first origin is measured cell by cell, past its bar the
// better of it and the second one is taken, a block neither serves is refused (status 2: its element vectors stay 0; the library refuses the whole plan)
static void run_p1(int nc, int block, const std::vector<double>& xc, const std::vector<int32_t>& cd, const std::vector<float>& u,
                   std::vector<float>& out, std::vector<int32_t>& status)
{
  auto points = [&](int c, double (&p)[4][3]) {
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a)
        p[k][a] = xc[(size_t)c * 12 + 3 * k + a];
  };
  for (int c0 = 0; c0 < nc; c0 += block)
  {
    const int c1 = c0 + block < nc ? c0 + block : nc;
    double o[3] = {xc[(size_t)c0 * 12], xc[(size_t)c0 * 12 + 1], xc[(size_t)c0 * 12 + 2]}, p[4][3];
    double o2[3] = {0.0, 0.0, 0.0};
    auto verdict = [&](const double (&org)[3], bool& ok, double& jerr) {
      ok = true;
      jerr = 0.0;
      for (int c = c0; c < c1; ++c)
      {
        points(c, p);
        const MfF32Verdict v = mf_f32_cell(p, org);
        ok = v.ok && ok;
        jerr = v.jerr > jerr ? v.jerr : jerr;
      }
    };
    bool ok0, ok1;
    double j0, j1;
    verdict(o, ok0, j0);
    int st = 0;
    if (!mf_f32_keep_first(ok0, j0, MF_F32_JTOL))
    {
      MfF32Thin t;
      for (int c = c0; c < c1; ++c)
      {
        points(c, p);
        mf_f32_thin_ext(t, p);
      }
      for (int c = c0; c < c1; ++c)
      {
        points(c, p);
        mf_f32_thin_at(t, p);
      }
      for (int a = 0; a < 3; ++a)
        o2[a] = t.at[a];
      verdict(o2, ok1, j1);
      st = mf_f32_choose(ok0, j0, ok1, j1, MF_F32_JTOL);
      if (st == 1)
        for (int a = 0; a < 3; ++a)
          o[a] = o2[a];
    }
    status.push_back(st);
    for (int c = c0; c < c1 && st != 2; ++c)
    {
      MfPoint<float> q[4];
      for (int k = 0; k < 4; ++k)
      {
        const double* v = &xc[(size_t)c * 12 + 3 * k];
        q[k] = {mf_rel_coord<float>(v[0], o[0]), mf_rel_coord<float>(v[1], o[1]), mf_rel_coord<float>(v[2], o[2]),
                u[(size_t)cd[(size_t)c * 4 + k]]};
      }
      float ye[4];
      mf_element_p1<false, float>(q[0], q[1], q[2], q[3], ye);
      for (int j = 0; j < 4; ++j)
        out[(size_t)c * 4 + j] = ye[j];
    }
  }
}

int main(int argc, char** argv)
{
  if (argc != 3 && argc != 4)
    return std::fprintf(stderr, "usage: %s IN OUT [STATUS]\n", argv[0]), 2;
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
  std::vector<int32_t> status; // P1: per block, 0 first origin, 1 second origin, 2 refused
  if (order == 1)
    run_p1(nc, block, xc, cd, u, out, status);
  else if (order == 2)
    run_pk<10>(ZZZ_DTAB_P2, nc, xc, cd, u, out);
  else
    run_pk<20>(ZZZ_DTAB_P3, nc, xc, cd, u, out);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size())
    return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  std::fclose(f);
  if (argc == 4)
  {
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(status.data(), 4, status.size(), f) != status.size())
      return std::fprintf(stderr, "cannot write %s\n", argv[3]), 2;
    std::fclose(f);
  }
  return 0;
}
