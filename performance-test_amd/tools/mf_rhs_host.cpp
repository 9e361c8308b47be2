// The per-cell arithmetic of the cell-block right-hand side (csrc/zzz_mf_elem.h: mf_rhs_mass, mf_rhs_mass3, mf_rhs_facet;
// csrc/zzz_cell_geom.h: geometry, facet_vertices, facet_scale_of -- what a lane of k_mf_rhs runs) on the CPU, cell by cell over a feed read from a file, in the manner of mf_f32_host.cpp: a
// stand-alone program that tests/test_mf_rhs_host_program.py builds with -fsanitize=address,undefined,float-divide-by-zero.
//
//   mf_rhs_host IN OUT
//
// IN:  int32 order, ncells, ndofs (block dofs), bs (1: Poisson's L, 3: elasticity's L);
//      double x[ncells][4][3]        the cells' vertices
//      int32  cell_dofs[ncells][nd]  block dofs
//      uint8  facet_mask[ncells]     bit lf = facet lf is exterior (bs 1; present and ignored for bs 3)
//      double f[ndofs * bs]          the coefficient f
//      double g[ndofs]               the boundary coefficient g (bs 1 only)
// OUT: double ye[ncells][nd][bs]     the element vectors; the caller scatters them and zeroes the constrained rows
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zzz_cell_geom.h"
#include "zzz_mf_elem.h"

namespace
{
template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <int ND>
int run(const double* tab, int bs, int ncells, const std::vector<double>& x, const std::vector<int32_t>& cd,
        const std::vector<uint8_t>& mask, const std::vector<double>& f, const std::vector<double>& g, std::vector<double>& out)
{
  const double* M = tab + 9 * ND * ND;
  const double* F = tab + 10 * ND * ND;
  out.assign((size_t)ncells * ND * bs, 0.0);
  for (int c = 0; c < ncells; ++c)
  {
    double p[4][3];
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a)
        p[k][a] = x[((size_t)c * 4 + k) * 3 + a];
    zzz::Geom G;
    zzz::geometry(p, G); // (|det J| as the kernel takes it)
    const int32_t* d = cd.data() + (size_t)c * ND;
    if (bs == 3)
    {
      double ye[3][ND];
      zzz::mf_rhs_mass3<ND>(M, G.adet, [&](int j, int comp, int) { return f[3 * (size_t)d[j] + comp]; }, ye);
      for (int j = 0; j < ND; ++j)
        for (int comp = 0; comp < 3; ++comp)
          out[((size_t)c * ND + j) * 3 + comp] = ye[comp][j];
    }
    else
    {
      double ye[ND];
      zzz::mf_rhs_mass<ND>(M, G.adet, [&](int j, int) { return f[(size_t)d[j]]; }, ye);
      for (int lf = 0; lf < 4; ++lf)
        if ((mask[(size_t)c] >> lf) & 1)
        {
          // the facet's three vertices alone, as the kernel fetches them
          int q[3];
          zzz::facet_vertices(lf, q[0], q[1], q[2]);
          double v[3][3];
          for (int t = 0; t < 3; ++t)
            for (int a = 0; a < 3; ++a)
              v[t][a] = p[q[t]][a];
          zzz::mf_rhs_facet<ND>(F, lf, zzz::facet_scale_of(v), [&](int j) { return g[(size_t)d[j]]; }, ye);
        }
      for (int j = 0; j < ND; ++j)
        out[(size_t)c * ND + j] = ye[j];
    }
  }
  return 0;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi)
  {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int32_t hdr[4];
  if (fread(hdr, sizeof(int32_t), 4, fi) != 4)
  {
    fprintf(stderr, "short header\n");
    fclose(fi);
    return 2;
  }
  const int order = hdr[0], ncells = hdr[1], ndofs = hdr[2], bs = hdr[3];
  const int nd = order == 1 ? 4 : (order == 2 ? 10 : (order == 3 ? 20 : 0));
  if (nd == 0 || ncells < 0 || ndofs <= 0 || (bs != 1 && bs != 3))
  {
    fprintf(stderr, "bad header\n");
    fclose(fi);
    return 2;
  }
  std::vector<double> x, f, g, out;
  std::vector<int32_t> cd;
  std::vector<uint8_t> mask;
  const bool ok = read_n(fi, x, (size_t)ncells * 12) && read_n(fi, cd, (size_t)ncells * nd) && read_n(fi, mask, (size_t)ncells)
                  && read_n(fi, f, (size_t)ndofs * bs) && read_n(fi, g, bs == 1 ? (size_t)ndofs : 0);
  fclose(fi);
  if (!ok)
  {
    fprintf(stderr, "short feed\n");
    return 2;
  }
  for (int32_t d : cd)
    if (d < 0 || d >= ndofs)
    {
      fprintf(stderr, "dof out of range\n");
      return 2;
    }
  if (nd == 4)
    run<4>(ZZZ_TAB_P1, bs, ncells, x, cd, mask, f, g, out);
  else if (nd == 10)
    run<10>(ZZZ_TAB_P2, bs, ncells, x, cd, mask, f, g, out);
  else
    run<20>(ZZZ_TAB_P3, bs, ncells, x, cd, mask, f, g, out);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo || (out.size() && fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()))
  {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    if (fo)
      fclose(fo);
    return 2;
  }
  fclose(fo);
  return 0;
}
