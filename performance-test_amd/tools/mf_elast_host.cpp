// The per-cell code of the matrix-free ELASTICITY action (csrc/zzz_mf_elem.h: mf_el_element_p1, mf_el_modes / _stress /
// _accumulate, mf_el_diag_pk, mf_cell_geom_el -- what the lanes of k_mf_action3 run) on the CPU, for runs under the sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ../csrc mf_elast_host.cpp -o mf_elast_host
//   mf_elast_host IN.txt
//
// IN.txt (numbers separated by white space): order ncells nnodes diag(0|1); then per cell its four vertices' coordinates
// (12 numbers); then per cell its nd node numbers; then u, 3 numbers per node (read also when diag = 1).
// Output: one line per cell with the 3 nd element results ye[j][c] (%.17g), the element vector A_e u_e or, diag = 1, the
// element matrix's diagonal.  tests/test_mf_elasticity_host.py scatters them and compares with the assembled matrix.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "zzz_mf_elem.h"

using namespace zzz;

template <int ND>
static void cell_pk(const double* dtab, const double (&p)[4][3], const int* dofs, const std::vector<double>& u, bool diag,
                    double (&ye)[3][ND])
{
  constexpr int NQ = MfTab<ND>::NQ, NT = 3 * NQ * ND;
  std::vector<double> tabT(NT);
  for (int k = 0; k < NT; ++k) // the kernel's second layout: [q][j][a]
  {
    const int a = k / (NQ * ND), q = (k / ND) % NQ, j = k % ND;
    tabT[(q * ND + j) * 3 + a] = dtab[k];
  }
  double Kd[10];
  mf_cell_geom_el(p, Kd);
  if (diag)
  {
    mf_el_diag_pk<ND>(tabT.data(), Kd, ye);
    return;
  }
  double g[3][NQ][3];
  for (int c = 0; c < 3; ++c)
  {
    double ue[ND];
    for (int j = 0; j < ND; ++j)
      ue[j] = u[3 * (size_t)dofs[j] + c];
    mf_el_modes<ND>(dtab, ue, g[c]);
  }
  mf_el_stress<NQ>(Kd, g);
  for (int c = 0; c < 3; ++c)
    mf_el_accumulate<ND>(tabT.data(), g[c], ye[c]);
}

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    fprintf(stderr, "usage: mf_elast_host IN.txt\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f)
  {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int order = 0, nc = 0, nn = 0, diag = 0;
  if (fscanf(f, "%d %d %d %d", &order, &nc, &nn, &diag) != 4 || order < 1 || order > 3 || nc < 1 || nn < 1)
  {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const int nd = order == 1 ? 4 : (order == 2 ? 10 : 20);
  std::vector<double> xc((size_t)nc * 12), u((size_t)nn * 3);
  std::vector<int> cd((size_t)nc * nd);
  bool ok = true;
  for (double& v : xc)
    ok = ok && fscanf(f, "%lf", &v) == 1;
  for (int& v : cd)
    ok = ok && fscanf(f, "%d", &v) == 1 && v >= 0 && v < nn;
  for (double& v : u)
    ok = ok && fscanf(f, "%lf", &v) == 1;
  fclose(f);
  if (!ok)
  {
    fprintf(stderr, "bad input\n");
    return 2;
  }
  for (int c = 0; c < nc; ++c)
  {
    double p[4][3];
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a)
        p[k][a] = xc[(size_t)c * 12 + 3 * k + a];
    const int* dofs = cd.data() + (size_t)c * nd;
    if (order == 1)
    {
      double uu[4][3], ye[4][3];
      for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a)
          uu[k][a] = u[3 * (size_t)dofs[k] + a];
      if (diag)
        mf_el_element_p1<true>(p, uu, ye);
      else
        mf_el_element_p1<false>(p, uu, ye);
      for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a)
          printf("%.17g ", ye[k][a]);
    }
    else if (order == 2)
    {
      double ye[3][10];
      cell_pk<10>(ZZZ_DTAB_P2, p, dofs, u, diag != 0, ye);
      for (int j = 0; j < 10; ++j)
        for (int a = 0; a < 3; ++a)
          printf("%.17g ", ye[a][j]);
    }
    else
    {
      double ye[3][20];
      cell_pk<20>(ZZZ_DTAB_P3, p, dofs, u, diag != 0, ye);
      for (int j = 0; j < 20; ++j)
        for (int a = 0; a < 3; ++a)
          printf("%.17g ", ye[a][j]);
    }
    printf("\n");
  }
  return 0;
}
