// Stand-alone check of the chunk planner with the costs of ghicp_gicp_clouds (gh_gicp_plan, gh-icp_amd/csrc/refine_plan.h); built with
// -fsanitize=address,undefined by tests/test_gicp_clouds_cpu.py.  The cases of test_refine_plan.cpp with the GICP costs: every plan must
// start at 0, end at n_pairs, grow strictly, and respect the chunk size asked for.  The plan of ghicp_refine_clouds must be what it was.
#include <cstdio>
#include <cstdlib>

#include "refine_plan.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static void well_formed(const std::vector<int>& b, int n) {
  CHECK(!b.empty() && b.front() == 0 && b.back() == (n > 0 ? n : 0));
  for (size_t i = 1; i < b.size(); i++) CHECK(b[i] > b[i - 1]);
}

int main() {
  const size_t big = (size_t)1 << 40;
  // per point the 48 B Mahalanobis matrix on top of the ICP batch's arrays; per pair no select histograms
  CHECK(kGicpPointBytes == kRefinePointBytes + 48);
  CHECK(kGicpPairBytes == kRefinePairBytes - 6 * 2048 * 4);
  // empty pair lists: with and without an array
  well_formed(gh_gicp_plan(0, nullptr, 0, big), 0);
  well_formed(gh_gicp_plan(0, nullptr, 3, big), 0);
  CHECK(gh_gicp_plan(0, nullptr, 0, 0).size() == 1);
  std::vector<int64_t> none;
  CHECK(gh_gicp_plan(0, none.data(), 1, big).size() == 1);
  for (int n : {1, 2, 5, 7, 64}) {
    std::vector<int64_t> ns((size_t)n);
    for (int i = 0; i < n; i++) ns[(size_t)i] = 1000 + 37 * i;
    for (int mc : {0, 1, 2, n, n + 1}) {
      const std::vector<int> b = gh_gicp_plan(n, ns.data(), mc, big);
      well_formed(b, n);
      if (mc == 0 || mc >= n) CHECK(b.size() == 2);  // everything in one chunk
      else {
        CHECK((int)b.size() - 1 == (n + mc - 1) / mc);
        for (size_t i = 1; i + 1 < b.size(); i++) CHECK(b[i] - b[i - 1] == mc);
        CHECK(b.back() - b[b.size() - 2] <= mc);
      }
    }
    // a budget that holds two pairs at the GICP costs: the automatic plan cuts there; one byte less and it cuts after the first pair
    const size_t two = 2 * kGicpPairBytes + kGicpPointBytes * (size_t)(ns[0] + ns[n > 1 ? 1 : 0]);
    const std::vector<int> b2 = gh_gicp_plan(n, ns.data(), 0, two);
    well_formed(b2, n);
    if (n >= 2) {
      CHECK(b2[1] == 2);
      CHECK(gh_gicp_plan(n, ns.data(), 0, two - 1)[1] == 1);
    }
    const std::vector<int> b0 = gh_gicp_plan(n, ns.data(), 0, 0);
    well_formed(b0, n);
    CHECK((int)b0.size() == n + 1);
    // an explicit chunk size is a memory knob of the caller: the budget does not override it
    const std::vector<int> bx = gh_gicp_plan(n, ns.data(), n, 0);
    CHECK(bx.size() == 2);
    // the four-argument call plans with the costs of ghicp_refine_clouds, as before
    const size_t two_rf = 2 * kRefinePairBytes + kRefinePointBytes * (size_t)(ns[0] + ns[n > 1 ? 1 : 0]);
    const std::vector<int> r2 = gh_refine_plan(n, ns.data(), 0, two_rf);
    well_formed(r2, n);
    if (n >= 2) {
      CHECK(r2[1] == 2);
      CHECK(gh_refine_plan(n, ns.data(), 0, two_rf - 1)[1] == 1);
    }
    CHECK(gh_refine_plan(n, ns.data(), 0, two_rf) == gh_refine_plan(n, ns.data(), 0, two_rf, kRefinePairBytes, kRefinePointBytes));
  }
  {  // more pairs than one status record holds; empty sources
    const int n = 2 * kRefineMaxChunk + 1;
    std::vector<int64_t> ns((size_t)n, 0);
    const std::vector<int> b = gh_gicp_plan(n, ns.data(), 0, big);
    well_formed(b, n);
    CHECK(b.size() == 4 && b[1] == kRefineMaxChunk);
    const std::vector<int> c = gh_gicp_plan(n, ns.data(), 1 << 30, big);
    CHECK(c.size() == 4);
  }
  printf(fails ? "gicp_plan: %d checks failed\n" : "gicp_plan ok\n", fails);
  return fails ? 1 : 0;
}
