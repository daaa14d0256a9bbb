// Stand-alone check of the grid plan and the budget rule behind ghicp_refine_clouds_reciprocal (gh-icp_amd/csrc/refine_recip_plan.h); built with
// -fsanitize=address,undefined by tests/test_refine_reciprocal_cpu.py.  For every box and budget: the grid fits the budget, its cell is
// never smaller than the one asked for, every point inside the box maps to a cell of the grid; the ranges of a chunk tile the table.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "refine_plan.h"
#include "refine_recip_plan.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void check_grid(const float* mm, float cell, unsigned budget) {
  const RecipGrid g = gh_recip_grid(mm, cell, budget);
  CHECK(g.dim[0] >= 1 && g.dim[1] >= 1 && g.dim[2] >= 1);
  CHECK((unsigned long long)g.dim[0] * g.dim[1] * g.dim[2] == g.ncell);
  CHECK(g.ncell >= 1 && g.ncell <= budget);
  CHECK(g.inv <= 1.0f / cell);  // the cell that came out is at least the one asked for
  for (int d = 0; d < 3; d++) CHECK(g.mn[d] == mm[d]);
  // the corners, the centre and a sweep of points of the box: each lands in a cell of the grid, and so does its key
  for (int k = 0; k <= 64; k++) {
    float P[3];
    for (int d = 0; d < 3; d++) {
      const float t = (float)((k * (d + 3)) % 65) / 64.0f;
      P[d] = mm[d] + t * (mm[3 + d] - mm[d]);
      if (P[d] > mm[3 + d]) P[d] = mm[3 + d];
    }
    if (k == 64) for (int d = 0; d < 3; d++) P[d] = mm[3 + d];
    int c[3];
    for (int d = 0; d < 3; d++) {
      c[d] = gh_recip_coord(P[d], g.mn[d], g.inv, g.dim[d]);
      CHECK(c[d] >= 0 && c[d] < g.dim[d]);
    }
    const unsigned key = ((unsigned)c[0] * g.dim[1] + c[1]) * g.dim[2] + c[2];
    CHECK(key < g.ncell);
  }
}

int main() {
  // ---- the grid of one pair
  const float boxes[][6] = {
      {0, 0, 0, 0, 0, 0},                          // zero extent: one point, or every point the same
      {-3.5f, 2, 1, -3.5f, 2, 1},
      {1, 0, 0, 66, 0, 0},                         // a line along one axis
      {0, 0, 0, 0, 0, 1e4f},
      {0, 0, 0, 7, 7, 3},                          // a small lattice
      {-40, -35, -2, 55, 48, 19},                  // a scan
      {-1e5f, -1e5f, -1e5f, 1e5f, 1e5f, 1e5f},     // huge extents
      {0, 0, 0, 3e37f, 1, 1},
      {-3e38f, -3e38f, -3e38f, 3e38f, 3e38f, 3e38f},  // the extent itself overflows
      {100000, 100000, 100000, 100001, 100001, 100001},  // far from the origin
  };
  const float cells[] = {0.02f, 0.1f, 0.37f, 1.0f, 2.5f, 8.0f, 100.0f};
  const unsigned budgets[] = {1u, 2u, 7u, 64u, 65u, 1000u, 16448u, 1u << 20, 1u << 30};
  for (const auto& b : boxes)
    for (float c : cells)
      for (unsigned q : budgets) check_grid(b, c, q);
  {  // a budget that is large enough leaves the cell as asked for (below the widening of long axes)
    const float mm[6] = {0, 0, 0, 7, 7, 3};
    const RecipGrid g = gh_recip_grid(mm, 1.0f, 1u << 20);
    CHECK(g.inv == 1.0f && g.dim[0] == 8 && g.dim[1] == 8 && g.dim[2] == 4 && g.ncell == 256);
    const RecipGrid h = gh_recip_grid(mm, 1.0f, 64);  // 1.5 x: 5 x 5 x 3 = 75; 2.25 x: 4 x 4 x 2 = 32
    CHECK(h.ncell <= 64 && h.inv < 1.0f && h.ncell == 32);
  }
  {  // a box that is not a number ends as one cell
    const float nan = std::nanf("");
    const float mm[6] = {0, 0, 0, nan, 1, 1};
    const RecipGrid g = gh_recip_grid(mm, 1.0f, 1000);
    CHECK(g.ncell == 1 && g.dim[0] == 1 && g.dim[1] == 1 && g.dim[2] == 1);
    CHECK(gh_recip_coord(nan, 0.f, g.inv, 1) == 0);
  }
  // ---- the ranges of a chunk
  auto check_ranges = [](const std::vector<int>& ns) {
    const int np = (int)ns.size();
    std::vector<RecipRange> r((size_t)np);
    const unsigned long long total = gh_recip_ranges(np, ns.data(), r.data());
    CHECK(total <= kRecipMaxCells);
    unsigned long long at = 0;
    for (int p = 0; p < np; p++) {  // the fine ranges tile the front of the table in pair order ...
      CHECK(r[(size_t)p].base_f == at && r[(size_t)p].cells_f >= kRecipMinCells);
      at += r[(size_t)p].cells_f;
    }
    for (int p = 0; p < np; p++) {  // ... the coarse ranges the rest: no two ranges overlap, nothing is left over
      CHECK(r[(size_t)p].base_c == at && r[(size_t)p].cells_c >= kRecipMinCells);
      at += r[(size_t)p].cells_c;
    }
    CHECK(at == total);
    return total;
  };
  CHECK(check_ranges({}) == 0);
  CHECK(check_ranges({0}) == 2 * kRecipMinCells);
  CHECK(check_ranges({-5, 0}) == 4 * kRecipMinCells);
  CHECK(check_ranges({255, 256, 257}) == (unsigned long long)(255 + 256 + 257) * (kRecipFineCells + kRecipCoarseCells) + 6 * kRecipMinCells);
  {
    std::vector<int> ns;
    for (int i = 0; i < 56; i++) ns.push_back(40000 + 977 * i);
    const unsigned long long total = check_ranges(ns);
    // what gh_refine_plan charges a chunk for covers its table
    size_t charged = 0;
    for (int n : ns) charged += kRecipPairBytes + kRecipPointBytes * (size_t)n;
    CHECK(total * 4 <= charged);
  }
  check_ranges(std::vector<int>(kRefineMaxChunk, 0));
  check_ranges(std::vector<int>(kRefineMaxChunk, 3));
  {  // more points than the table may have cells for at the full multiples: the multiples are halved, every range keeps its minimum
    std::vector<int> big(64, 2000000000);
    std::vector<RecipRange> r(big.size());
    const unsigned long long total = gh_recip_ranges((int)big.size(), big.data(), r.data());
    CHECK(total <= kRecipMaxCells && r[0].cells_f >= kRecipMinCells && r[63].cells_c >= kRecipMinCells);
    check_ranges(big);
    check_ranges({2147483645});
    check_ranges({20000000, 1, 20000000});
  }
  // the plan of the other loops is what it was
  CHECK(kRecipPointBytes > kRefinePointBytes && kRecipPairBytes > kRefinePairBytes);
  printf(fails ? "refine_recip_plan: %d checks failed\n" : "refine_recip_plan ok\n", fails);
  return fails ? 1 : 0;
}
