// csrc/zzz_mg_transfer.h on the CPU, a stand-alone program for a sanitizer build (tests/test_mg_slab_host_program.py builds it
// with -fsanitize=address,undefined): the tables, the simplex and the two walks of ZZZ_PC_MG's grid transfer as the kernels of
// csrc/zzz_mg.hip run them, once on the whole cube and once per z-slab of a partition, every slab with vectors of exactly its own
// length (so a walk that leaves its window leaves its allocation).
//   * prolongation: the slabs' results, concatenated, are the whole-cube walk's bit for bit;
//   * restriction: every slab writes only the coarse planes [cz0, cz1] it says it reaches, and a walk over ALL coarse vertices
//     finds zero everywhere else; the rank-ordered sum of the partial restrictions stays within 1e-13 of max |out| of the whole
//     restriction (ZZZ_PC_MG's transfer bar: a sum of at most about 30 terms split in at most three places);
//   * the residual formed on the way in (sub != null) takes the same path.
// Usage: mg_slab_host <directory>.  Per case one file <directory>/case_<k>.bin: seven int64 {bs, nx, ny, nz, nparts, fine dofs,
// coarse dofs}, then the doubles e (coarse), r (fine), P e, the rank-ordered sum of the partial restrictions, the whole
// restriction.  Prints one line per case; exit status 0 and "ok" when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "zzz_mg_transfer.h"

using namespace zzz;

static int failures = 0;
#define CHECK(cond)                                                                              \
  do                                                                                             \
  {                                                                                              \
    if (!(cond))                                                                                 \
    {                                                                                            \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);             \
      ++failures;                                                                                \
    }                                                                                            \
  } while (0)

static double noise(uint64_t i, uint64_t salt)
{
  uint32_t h = (uint32_t)((i + salt * 1000003ull) * 2654435761ull + 12345ull);
  h ^= h >> 16;
  h *= 0x45d9f3bu;
  h ^= h >> 16;
  return (double)h / 4294967296.0 - 0.5;
}

// the Dirichlet bytes of the generated problems on n cells: Poisson x = 0 or 1, elasticity y = 0 (host/cube_layout.h)
static std::vector<uint8_t> dirichlet(int bs, const int64_t n[3])
{
  const int64_t px = n[0] + 1, py = n[1] + 1, pz = n[2] + 1;
  std::vector<uint8_t> bc((size_t)(px * py * pz * bs), 0);
  for (int64_t v = 0; v < px * py * pz; ++v)
  {
    const int64_t ix = v % px, iy = (v / px) % py;
    const bool on = bs == 1 ? (ix == 0 || ix == n[0]) : iy == 0;
    for (int k = 0; k < bs; ++k)
      bc[(size_t)(v * bs + k)] = on ? 1 : 0;
  }
  return bc;
}

struct Tables
{
  MgGeom G;
  std::vector<int32_t> tc, rng;
  std::vector<double> tf;
  Tables(const int64_t nf[3], const int64_t nc[3], int bs, int64_t z0, int64_t z1)
  {
    int64_t a = 0, b = 0;
    mg_table_sizes(nf, nc, &a, &b);
    tc.resize((size_t)a);
    tf.resize((size_t)a);
    rng.resize(2 * (size_t)b);
    mg_fill_tables(G, nf, nc, bs, z0, z1, tc.data(), tf.data(), rng.data());
  }
};

static void restrict_all(const Tables& T, int bs, const uint8_t* bcf, const uint8_t* bcc, const double* rf, const double* sub, double* rc,
                         int64_t c_begin, int64_t c_end)
{
  for (int64_t c = c_begin; c < c_end; ++c)
    if (bs == 3)
      mg_restrict_vertex<3>(T.G, T.tc.data(), T.tf.data(), T.rng.data(), bcf, bcc, rf, sub, rc, c);
    else
      mg_restrict_vertex<1>(T.G, T.tc.data(), T.tf.data(), T.rng.data(), bcf, bcc, rf, sub, rc, c);
}

static void run_case(int k, const std::string& dir, int bs, int64_t nx, int64_t ny, int64_t nz, int nparts)
{
  const int64_t nf[3] = {nx, ny, nz};
  int64_t nc[3];
  for (int a = 0; a < 3; ++a)
    nc[a] = (nf[a] + 1) / 2 > 2 ? (nf[a] + 1) / 2 : 2;
  const int64_t plane = (nx + 1) * (ny + 1), nfine = plane * (nz + 1) * bs, cplane = (nc[0] + 1) * (nc[1] + 1),
                ncoarse = cplane * (nc[2] + 1) * bs;
  const std::vector<uint8_t> bcf = dirichlet(bs, nf), bcc = dirichlet(bs, nc);
  std::vector<double> e((size_t)ncoarse), r((size_t)nfine), ax((size_t)nfine);
  for (int64_t i = 0; i < ncoarse; ++i)
    e[(size_t)i] = noise((uint64_t)i, 1);
  for (int64_t i = 0; i < nfine; ++i)
  {
    r[(size_t)i] = noise((uint64_t)i, 2);
    ax[(size_t)i] = noise((uint64_t)i, 3);
  }
  // the whole cube: the window [0, nz]
  const Tables W(nf, nc, bs, 0, nz);
  CHECK(W.G.nfv * bs == nfine && W.G.ncv * bs == ncoarse && W.G.cz0 == 0 && W.G.cz1 == nc[2]);
  std::vector<double> pe((size_t)nfine, 7.0), pacc((size_t)nfine), rt((size_t)ncoarse, 7.0), rts((size_t)ncoarse, 7.0);
  for (int64_t i = 0; i < nfine; ++i)
    pacc[(size_t)i] = r[(size_t)i];
  for (int64_t v = 0; v < W.G.nfv; ++v)
  {
    mg_prolong_vertex(W.G, W.tc.data(), W.tf.data(), bcf.data(), bcc.data(), e.data(), pe.data(), 0, v);
    mg_prolong_vertex(W.G, W.tc.data(), W.tf.data(), bcf.data(), bcc.data(), e.data(), pacc.data(), 1, v);
  }
  restrict_all(W, bs, bcf.data(), bcc.data(), r.data(), nullptr, rt.data(), 0, W.G.ncv);
  restrict_all(W, bs, bcf.data(), bcc.data(), r.data(), ax.data(), rts.data(), 0, W.G.ncv);
  // the slabs, each with vectors of its own length
  std::vector<double> sum((size_t)ncoarse, 0.0), sums((size_t)ncoarse, 0.0);
  int64_t next_plane = 0, widest = 0;
  for (int p = 0; p < nparts; ++p)
  {
    int64_t p0 = 0, p1 = 0;
    mg_slab_planes(nz, nparts, p, &p0, &p1);
    CHECK(p0 == next_plane && p1 >= p0 && p1 <= nz); // the parts own every plane once, in order
    next_plane = p1 + 1;
    const Tables S(nf, nc, bs, p0, p1);
    const int64_t nown = plane * (p1 - p0 + 1) * bs, off = plane * p0 * bs;
    CHECK(S.G.nfv * bs == nown && S.G.cz0 >= 0 && S.G.cz1 <= nc[2] && S.G.cz0 <= S.G.cz1);
    widest = S.G.cz1 - S.G.cz0 + 1 > widest ? S.G.cz1 - S.G.cz0 + 1 : widest;
    const std::vector<uint8_t> bcs(bcf.begin() + off, bcf.begin() + off + nown);
    const std::vector<double> rs(r.begin() + off, r.begin() + off + nown), axs(ax.begin() + off, ax.begin() + off + nown);
    std::vector<double> xs((size_t)nown, 7.0), xacc(rs);
    for (int64_t v = 0; v < S.G.nfv; ++v)
    {
      mg_prolong_vertex(S.G, S.tc.data(), S.tf.data(), bcs.data(), bcc.data(), e.data(), xs.data(), 0, v);
      mg_prolong_vertex(S.G, S.tc.data(), S.tf.data(), bcs.data(), bcc.data(), e.data(), xacc.data(), 1, v);
    }
    CHECK(std::memcmp(xs.data(), pe.data() + off, (size_t)nown * sizeof(double)) == 0);
    CHECK(std::memcmp(xacc.data(), pacc.data() + off, (size_t)nown * sizeof(double)) == 0);
    // the kernel's form: the reached planes by the walk, zero elsewhere
    std::vector<double> part((size_t)ncoarse, 0.0), parts((size_t)ncoarse, 0.0), every((size_t)ncoarse, 7.0);
    const int64_t c0 = S.G.cz0 * cplane;
    restrict_all(S, bs, bcs.data(), bcc.data(), rs.data(), nullptr, part.data(), c0, c0 + S.G.ncv);
    restrict_all(S, bs, bcs.data(), bcc.data(), rs.data(), axs.data(), parts.data(), c0, c0 + S.G.ncv);
    // ... and over every coarse vertex: the planes outside [cz0, cz1] get nothing from this slab
    restrict_all(S, bs, bcs.data(), bcc.data(), rs.data(), nullptr, every.data(), 0, cplane * (nc[2] + 1));
    CHECK(std::memcmp(every.data(), part.data(), (size_t)ncoarse * sizeof(double)) == 0);
    for (int64_t i = 0; i < ncoarse; ++i)
    {
      sum[(size_t)i] += part[(size_t)i]; // rank order
      sums[(size_t)i] += parts[(size_t)i];
    }
  }
  CHECK(next_plane == nz + 1);
  double top = 0.0, dmax = 0.0, tops = 0.0, dmaxs = 0.0;
  for (int64_t i = 0; i < ncoarse; ++i)
  {
    top = std::fmax(top, std::fabs(rt[(size_t)i]));
    dmax = std::fmax(dmax, std::fabs(sum[(size_t)i] - rt[(size_t)i]));
    tops = std::fmax(tops, std::fabs(rts[(size_t)i]));
    dmaxs = std::fmax(dmaxs, std::fabs(sums[(size_t)i] - rts[(size_t)i]));
  }
  CHECK(top > 0.0 && dmax <= 1e-13 * top);
  CHECK(tops > 0.0 && dmaxs <= 1e-13 * tops);
  std::printf("case %d: bs %d, %lldx%lldx%lld on %d parts: restriction sum off by %.2e of max |out| (with the residual %.2e), widest reach "
              "%lld of %lld coarse planes\n", k, bs, (long long)nx, (long long)ny, (long long)nz, nparts, dmax / top, dmaxs / tops,
              (long long)widest, (long long)(nc[2] + 1));
  const std::string path = dir + "/case_" + std::to_string(k) + ".bin";
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f)
  {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    ++failures;
    return;
  }
  const int64_t head[7] = {bs, nx, ny, nz, nparts, nfine, ncoarse};
  bool ok = std::fwrite(head, sizeof(int64_t), 7, f) == 7;
  ok = ok && std::fwrite(e.data(), sizeof(double), e.size(), f) == e.size();
  ok = ok && std::fwrite(r.data(), sizeof(double), r.size(), f) == r.size();
  ok = ok && std::fwrite(pe.data(), sizeof(double), pe.size(), f) == pe.size();
  ok = ok && std::fwrite(sum.data(), sizeof(double), sum.size(), f) == sum.size();
  ok = ok && std::fwrite(rt.data(), sizeof(double), rt.size(), f) == rt.size();
  ok = std::fclose(f) == 0 && ok;
  CHECK(ok);
}

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    std::fprintf(stderr, "usage: %s <directory>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  int k = 0;
  // nested in z; not nested; slabs of one plane and the capped top coarse index; block size 3
  for (int np : {2, 3, 4})
    run_case(k++, dir, 1, 10, 9, 12, np);
  run_case(k++, dir, 1, 7, 6, 9, 3);
  run_case(k++, dir, 1, 6, 5, 3, 3);
  for (int np : {2, 4})
    run_case(k++, dir, 3, 5, 5, 8, np);
  if (failures)
  {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
