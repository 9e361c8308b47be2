// csrc/zzz_sagg_rows.h on the CPU, a stand-alone program for a sanitizer build (tests/test_sagg_rows_host_program.py builds it
// with -fsanitize=address,undefined): the chunk partition of the symbolic pass, the search of a column in a sorted output row
// and one small product C = L B formed row by row as the kernels of csrc/zzz_sagg_rows.hip form it -- one accumulator per
// output entry, the entries of L's row in order, each term finding its accumulator by the search -- against the order of the
// lists mode: every term written out in ascending summation index, stably sorted by (row, column), each run summed front to
// back.  The two must agree bit for bit, sign of zero included.  Exit status 0 and "ok" when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zzz_sagg_rows.h"

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

// the chunks of `cand` under `budget`: [start of every chunk ..., nrows]; checks the partition's promises on the way
static std::vector<int64_t> chunks_of(const std::vector<int64_t>& cand, int64_t budget, int64_t* lone)
{
  const int64_t n = (int64_t)cand.size();
  std::vector<int64_t> cum((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; ++r)
    cum[(size_t)r + 1] = cum[(size_t)r] + cand[(size_t)r];
  std::vector<int64_t> starts;
  *lone = 0;
  for (int64_t r0 = 0; r0 < n;)
  {
    const int64_t r1 = srow_chunk_end(cum.data(), n, r0, budget);
    CHECK(r1 > r0 && r1 <= n); // at least one row, ends on a row boundary inside the matrix
    const int64_t c = cum[(size_t)r1] - cum[(size_t)r0];
    if (c > budget)
    {
      CHECK(r1 == r0 + 1); // over the budget: that row alone
      ++*lone;
    }
    else if (r1 < n)
      CHECK(c + cand[(size_t)r1] > budget); // within it: the next row would not have fitted
    starts.push_back(r0);
    r0 = r1;
  }
  starts.push_back(n);
  return starts;
}

static void check_partition()
{
  int64_t lone = 0;
  // empty rows between the others, a total of zero, no row at all
  CHECK((chunks_of({0, 0, 3, 0, 4, 0, 0, 2, 0}, 5, &lone) == std::vector<int64_t>{0, 4, 7, 9}) && lone == 0);
  CHECK((chunks_of({0, 0, 0, 0}, 7, &lone) == std::vector<int64_t>{0, 4}) && lone == 0);
  CHECK((chunks_of({}, 7, &lone) == std::vector<int64_t>{0}) && lone == 0);
  // a row over the budget is a chunk of its own, wherever it stands (the empty row behind it opens the next chunk)
  CHECK((chunks_of({9, 1, 1, 9, 0, 1, 9}, 4, &lone) == std::vector<int64_t>{0, 1, 3, 4, 6, 7}) && lone == 3);
  // budget 1: a chunk per non-empty row
  CHECK((chunks_of({1, 1, 0, 2, 1}, 1, &lone) == std::vector<int64_t>{0, 1, 3, 4, 5}) && lone == 1);
  // 4 096 rows of 2^20 candidates: a total of 2^32, which 32-bit sums would wrap to zero
  {
    const std::vector<int64_t> cand(4096, 1ll << 20);
    const std::vector<int64_t> s = chunks_of(cand, (1ll << 24) + 5, &lone);
    CHECK(s.size() == 257 && lone == 0);
    for (size_t i = 0; i + 1 < s.size(); ++i)
      CHECK(s[i + 1] - s[i] == 16);
    const std::vector<int64_t> one = chunks_of(cand, 1ll << 33, &lone);
    CHECK((one == std::vector<int64_t>{0, 4096}));
    const std::vector<int64_t> each = chunks_of(cand, (1ll << 20) - 1, &lone);
    CHECK(each.size() == 4097 && lone == 4096);
  }
}

static void check_search()
{
  for (int n : {0, 1, 63, 64, 65})
  {
    std::vector<int32_t> cols((size_t)n);
    for (int j = 0; j < n; ++j)
      cols[(size_t)j] = 3 * j + 1; // ascending, distinct, with gaps
    for (int j = 0; j < n; ++j)
    {
      CHECK(srow_find(cols.data(), n, 3 * j + 1) == j);
      CHECK(srow_find(cols.data(), n, 3 * j) == -1 && srow_find(cols.data(), n, 3 * j + 2) == -1);
    }
    CHECK(srow_find(cols.data(), n, -5) == -1 && srow_find(cols.data(), n, 3 * n + 1) == -1);
    // (heap-allocated exactly: a read one past either end is the sanitizer's to report)
  }
  const int64_t a[5] = {0, 0, 4, 4, 9};
  CHECK(srow_upper_bound<int64_t>(a, 0, 5, -1) == 0 && srow_upper_bound<int64_t>(a, 0, 5, 0) == 2 && srow_upper_bound<int64_t>(a, 0, 5, 4) == 4);
  CHECK(srow_upper_bound<int64_t>(a, 0, 5, 9) == 5 && srow_upper_bound<int64_t>(a, 2, 2, 0) == 2);
}

struct Csr
{
  int64_t nrows = 0, ncols = 0;
  std::vector<int64_t> row;
  std::vector<int32_t> col;
  std::vector<double> val;
};

static uint64_t lcg(uint64_t& s)
{
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// rows of random length (some empty), ascending distinct columns; values of both signs, exact zeros and negative zeros among them
static Csr random_csr(int64_t nrows, int64_t ncols, int max_len, uint64_t seed)
{
  Csr M;
  M.nrows = nrows;
  M.ncols = ncols;
  M.row.push_back(0);
  uint64_t s = seed;
  for (int64_t r = 0; r < nrows; ++r)
  {
    const int len = (int)(lcg(s) % (uint64_t)(max_len + 1));
    std::vector<int32_t> c;
    for (int j = 0; j < len; ++j)
      c.push_back((int32_t)(lcg(s) % (uint64_t)ncols));
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    for (int32_t j : c)
    {
      const uint64_t k = lcg(s) % 16;
      const double v = k == 0 ? 0.0 : k == 1 ? -0.0 : ((double)(lcg(s) % 2000001) - 1000000.0) * 1e-6 * (k < 8 ? 1.0 : 1e-9);
      M.col.push_back(j);
      M.val.push_back(v);
    }
    M.row.push_back((int64_t)M.col.size());
  }
  return M;
}

static void check_product(int64_t budget)
{
  const Csr L = random_csr(97, 61, 23, 1), B = random_csr(61, 73, 70, 2);
  // ---- the lists mode's order: terms in ascending (row, summation index), stably sorted by (row, column), runs summed ----
  struct Term
  {
    uint64_t key;
    double a, b;
  };
  std::vector<Term> terms;
  for (int64_t r = 0; r < L.nrows; ++r)
    for (int64_t t = L.row[(size_t)r]; t < L.row[(size_t)r + 1]; ++t)
    {
      const int32_t k = L.col[(size_t)t];
      for (int64_t q = B.row[(size_t)k]; q < B.row[(size_t)k + 1]; ++q)
        terms.push_back({((uint64_t)r << 32) | (uint64_t)B.col[(size_t)q], L.val[(size_t)t], B.val[(size_t)q]});
    }
  std::stable_sort(terms.begin(), terms.end(), [](const Term& x, const Term& y) { return x.key < y.key; });
  std::vector<uint64_t> ref_key;
  std::vector<double> ref_val;
  for (size_t t = 0; t < terms.size();)
  {
    double s = 0.0;
    size_t e = t;
    for (; e < terms.size() && terms[e].key == terms[t].key; ++e)
      s = srow_add(s, terms[e].a, terms[e].b);
    ref_key.push_back(terms[t].key);
    ref_val.push_back(s);
    t = e;
  }
  // ---- row by row.  Symbolic: candidate counts, 64-bit prefix sums, chunks, sort + unique per chunk -----------------------
  std::vector<int64_t> cum((size_t)L.nrows + 1, 0);
  for (int64_t r = 0; r < L.nrows; ++r)
  {
    int64_t n = 0;
    for (int64_t t = L.row[(size_t)r]; t < L.row[(size_t)r + 1]; ++t)
      n += B.row[(size_t)L.col[(size_t)t] + 1] - B.row[(size_t)L.col[(size_t)t]];
    cum[(size_t)r + 1] = cum[(size_t)r] + n;
  }
  CHECK(cum[(size_t)L.nrows] == (int64_t)terms.size());
  Csr C;
  C.nrows = L.nrows;
  C.row.assign((size_t)L.nrows + 1, 0);
  int nchunks = 0;
  for (int64_t r0 = 0; r0 < L.nrows;)
  {
    const int64_t r1 = srow_chunk_end(cum.data(), L.nrows, r0, budget);
    std::vector<uint64_t> key((size_t)(cum[(size_t)r1] - cum[(size_t)r0])); // (exactly the chunk's candidates)
    for (int64_t r = r0; r < r1; ++r)
    {
      int64_t o = cum[(size_t)r] - cum[(size_t)r0];
      for (int64_t t = L.row[(size_t)r]; t < L.row[(size_t)r + 1]; ++t)
        for (int64_t q = B.row[(size_t)L.col[(size_t)t]]; q < B.row[(size_t)L.col[(size_t)t] + 1]; ++q)
          key[(size_t)o++] = ((uint64_t)r << 32) | (uint64_t)B.col[(size_t)q];
      CHECK(o == cum[(size_t)r + 1] - cum[(size_t)r0]);
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    for (uint64_t k : key)
    {
      C.col.push_back((int32_t)(k & 0xffffffffull));
      ++C.row[(size_t)(k >> 32) + 1];
    }
    ++nchunks;
    r0 = r1;
  }
  for (int64_t r = 0; r < L.nrows; ++r)
    C.row[(size_t)r + 1] += C.row[(size_t)r];
  CHECK(C.col.size() == ref_key.size());
  CHECK(budget < (int64_t)terms.size() ? nchunks > 1 : nchunks == 1);
  // ---- numeric: one accumulator per output entry, L's entries in order, the search gives the accumulator ------------------
  C.val.assign(C.col.size(), -1.0);
  for (int64_t r = 0; r < L.nrows; ++r)
  {
    const int64_t c0 = C.row[(size_t)r];
    const int32_t n = (int32_t)(C.row[(size_t)r + 1] - c0);
    // (n may be 0: data() + c0 is then never dereferenced)
    std::vector<int32_t> cc(C.col.begin() + c0, C.col.begin() + c0 + n);
    std::vector<double> acc((size_t)n, 0.0);
    for (int64_t t = L.row[(size_t)r]; t < L.row[(size_t)r + 1]; ++t)
    {
      const int32_t k = L.col[(size_t)t];
      for (int64_t q = B.row[(size_t)k]; q < B.row[(size_t)k + 1]; ++q)
      {
        const int32_t p = srow_find(cc.data(), n, B.col[(size_t)q]);
        CHECK(p >= 0);
        if (p >= 0)
          acc[(size_t)p] = srow_add(acc[(size_t)p], L.val[(size_t)t], B.val[(size_t)q]);
      }
    }
    std::copy(acc.begin(), acc.end(), C.val.begin() + c0);
  }
  size_t e = 0;
  bool same = C.col.size() == ref_key.size();
  for (int64_t r = 0; same && r < L.nrows; ++r)
    for (int64_t q = C.row[(size_t)r]; q < C.row[(size_t)r + 1]; ++q, ++e)
      same = same && ref_key[e] == (((uint64_t)r << 32) | (uint64_t)C.col[(size_t)q])
             && std::memcmp(&ref_val[e], &C.val[(size_t)q], sizeof(double)) == 0;
  CHECK(same);
  std::printf("product: budget %lld, %zu terms, %zu entries, %d chunks\n", (long long)budget, terms.size(), C.col.size(), nchunks);
}

int main()
{
  check_partition();
  check_search();
  check_product(1ll << 40);
  check_product(500);
  check_product(1);
  if (failures)
    return 1;
  std::printf("ok\n");
  return 0;
}
