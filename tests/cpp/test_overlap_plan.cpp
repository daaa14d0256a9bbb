// Stand-alone check of the chunk planner of ghicp_overlap_clouds and of the block -> pair search its kernel runs (gh_overlap_plan,
// gh_ov_pair_of_block, gh-icp_amd/csrc/overlap_plan.h); built with -fsanitize=address,undefined by tests/test_overlap_clouds_cpu.py.
// Every plan must cover the pairs in order without gaps; every block of a chunk must map back to the pair that owns it and to its block
// within that pair; pairs without blocks are never returned.
#include <cstdio>
#include <cstdlib>

#include "overlap_plan.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// the plan is well formed for ns, and every block index of every chunk maps back to (pair, block within the pair)
static void check_plan(const std::vector<OvChunk>& plan, const std::vector<int64_t>& ns) {
  const int n = (int)ns.size();
  CHECK(plan.empty() == (n == 0));
  int next = 0;
  for (const OvChunk& ch : plan) {
    CHECK(ch.p0 == next && ch.p1 > ch.p0 && ch.p1 <= n);
    next = ch.p1;
    const int np = ch.p1 - ch.p0;
    CHECK((int)ch.first.size() == np + 1 && ch.first[0] == 0);
    // each heap copy holds exactly np + 1 entries: a read past the table aborts under AddressSanitizer
    int* first = (int*)malloc((size_t)(np + 1) * sizeof(int));
    for (int q = 0; q <= np; q++) first[q] = ch.first[(size_t)q];
    for (int q = 0; q < np; q++) CHECK(first[q + 1] - first[q] == (int)((ns[(size_t)(ch.p0 + q)] + 255) / 256));
    int b = 0;
    for (int q = 0; q < np; q++) {
      const int nb = first[q + 1] - first[q];
      for (int k = 0; k < nb; k++, b++) {
        const int got = gh_ov_pair_of_block(first, np, b);
        CHECK(got == q);                        // the right pair, never a pair without blocks
        CHECK(b - first[got] == k);             // and the right block within it
        CHECK(ns[(size_t)(ch.p0 + got)] > 0);
        CHECK((long long)(b - first[got]) * 256 < ns[(size_t)(ch.p0 + got)]);  // the block's first point exists
      }
    }
    CHECK(b == first[np]);
    free(first);
  }
  CHECK(next == n);
}

int main() {
  const std::vector<int64_t> sizes = {257, 1, 0, 256, 513, 64, 0};
  const int n = (int)sizes.size();
  {  // one chunk: blocks 2 1 0 1 3 1 0
    const std::vector<OvChunk> plan = gh_overlap_plan(n, sizes.data(), 0);
    check_plan(plan, sizes);
    CHECK(plan.size() == 1);
    const std::vector<int> want = {0, 2, 3, 3, 4, 7, 8, 8};
    CHECK(plan[0].first == want);
    const int owner[8] = {0, 0, 1, 3, 4, 4, 4, 5};
    for (int b = 0; b < 8; b++) CHECK(gh_ov_pair_of_block(plan[0].first.data(), n, b) == owner[b]);
  }
  for (int mc : {0, 1, 2, n, n + 1}) {
    const std::vector<OvChunk> plan = gh_overlap_plan(n, sizes.data(), mc);
    check_plan(plan, sizes);
    if (mc == 0 || mc >= n) CHECK(plan.size() == 1);
    else {
      CHECK((int)plan.size() == (n + mc - 1) / mc);
      for (size_t c = 0; c + 1 < plan.size(); c++) CHECK(plan[c].p1 - plan[c].p0 == mc);
      CHECK(plan.back().p1 - plan.back().p0 <= mc);
    }
  }
  {  // an empty list, with and without an array
    CHECK(gh_overlap_plan(0, nullptr, 0).empty());
    CHECK(gh_overlap_plan(0, nullptr, 3).empty());
    std::vector<int64_t> none;
    check_plan(gh_overlap_plan(0, none.data(), 1), none);
  }
  {  // all-zero sizes: chunks without a block (the caller launches nothing for them)
    const std::vector<int64_t> zeros(5, 0);
    for (int mc : {0, 2}) {
      const std::vector<OvChunk> plan = gh_overlap_plan(5, zeros.data(), mc);
      check_plan(plan, zeros);
      for (const OvChunk& ch : plan) CHECK(ch.first.back() == 0);
    }
  }
  {  // a block cap that forces a split in the middle: 2 + 1 + 0 + 1 = 4 blocks fit a cap of 4, the 3 blocks of pair 4 do not
    const std::vector<OvChunk> plan = gh_overlap_plan(n, sizes.data(), 0, 4);
    check_plan(plan, sizes);
    CHECK(plan.size() == 2 && plan[0].p1 == 4 && plan[0].first.back() == 4 && plan[1].first.back() == 4);
    // a cap below a single pair's blocks: that pair gets a chunk of its own
    const std::vector<OvChunk> one = gh_overlap_plan(n, sizes.data(), 0, 1);
    check_plan(one, sizes);
    for (const OvChunk& ch : one) CHECK(ch.first.back() <= 3);
    CHECK(one.size() == 5);  // {257}, {1, 0}, {256}, {513}, {64, 0}
    // the cap and an explicit chunk size together: whichever closes the chunk first
    const std::vector<OvChunk> both = gh_overlap_plan(n, sizes.data(), 3, 4);
    check_plan(both, sizes);
    CHECK(both.size() == 3 && both[0].p1 == 3 && both[1].p1 == 5);  // {257, 1, 0} by the size, {256, 513} by the cap, {64, 0}
  }
  {  // more pairs than one launch holds
    const int m = 2 * kOvMaxChunk + 1;
    std::vector<int64_t> ns((size_t)m);
    for (int i = 0; i < m; i++) ns[(size_t)i] = (i % 3) * 200;
    const std::vector<OvChunk> plan = gh_overlap_plan(m, ns.data(), 0);
    check_plan(plan, ns);
    CHECK(plan.size() == 3 && plan[0].p1 == kOvMaxChunk);
    CHECK(gh_overlap_plan(m, ns.data(), 1 << 30).size() == 3);
  }
  printf(fails ? "overlap_plan: %d checks failed\n" : "overlap_plan ok\n", fails);
  return fails ? 1 : 0;
}
