// Internal: how ghicp_refine_clouds and ghicp_gicp_clouds cut their pairs into chunks (pairs that share one launch sequence).  Plain C++, no HIP: the planner is
// compiled on its own by tests/cpp/test_refine_plan.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "refine_recip_plan.h"

constexpr int kRefineMaxChunk = 4096;                    // one status byte per pair in the context's 4 KB pinned record
constexpr size_t kRefinePairBytes = 512 * 32 * 8         // the pair's NBLK partial records
                                    + 6 * 2048 * 4       // its radix-select histograms
                                    + 1024;              // descriptor, state, counters
constexpr size_t kRefinePointBytes = 16 + 4 + 4 + 4;     // cur, nn, nd, work list of the coarse search -- per source point
// ghicp_refine_clouds_reciprocal (refine_recip.hip) on top of that, per source point: the query and the back-search's nn / nd / work list, the
// point's index within its pair; every point enters the sort twice (fine and coarse key): keys and values double-buffered, the sort's spare
// pair, the points in cell order; the pair's ranges of the cell table (refine_recip_plan.h).  Per pair: the minimum ranges, its boxes and grids.
constexpr size_t kRecipPointBytes = kRefinePointBytes + 16 + 4 + 4 + 4 + 4 + 2 * (4 * 4) + 2 * (4 + 4) + 2 * 16 + 4 * (kRecipFineCells + kRecipCoarseCells);
constexpr size_t kRecipPairBytes = kRefinePairBytes + 2 * 4 * kRecipMinCells + 256;

// Chunk boundaries b[0] = 0 < b[1] < ... < b.back() = n_pairs over the pairs in the given order (empty list: {0}).  max_concurrent > 0: chunks of
// exactly that many pairs (the last one shorter), capped at kRefineMaxChunk.  0: as many pairs per chunk as fit `budget` bytes by the per-pair
// and per-point costs above, at least one.  ns[p]: source points of pair p.
// pair_bytes / point_bytes: the costs of the loop that is planned (defaults: ghicp_refine_clouds).
inline std::vector<int> gh_refine_plan(int n_pairs, const int64_t* ns, int max_concurrent, size_t budget, size_t pair_bytes = kRefinePairBytes,
                                       size_t point_bytes = kRefinePointBytes) {
  std::vector<int> b(1, 0);
  if (n_pairs <= 0) return b;
  const int cap = max_concurrent > 0 && max_concurrent < kRefineMaxChunk ? max_concurrent : kRefineMaxChunk;
  size_t used = 0;
  int in_chunk = 0;
  for (int p = 0; p < n_pairs; p++) {
    const size_t cost = pair_bytes + point_bytes * (size_t)(ns[p] > 0 ? ns[p] : 0);
    const bool full = in_chunk >= cap || (max_concurrent <= 0 && in_chunk > 0 && used + cost > budget);
    if (full) { b.push_back(p); used = 0; in_chunk = 0; }
    used += cost;
    in_chunk++;
  }
  b.push_back(n_pairs);
  return b;
}

// ghicp_gicp_clouds (refine_gicp.hip): per point the 48 B Mahalanobis matrix on top of cur / nn / nd / work list; per pair the partial records
// and a state record, no select histograms.
constexpr size_t kGicpPairBytes = 512 * 32 * 8 + 1024;
constexpr size_t kGicpPointBytes = kRefinePointBytes + 48;
inline std::vector<int> gh_gicp_plan(int n_pairs, const int64_t* ns, int max_concurrent, size_t budget) {
  return gh_refine_plan(n_pairs, ns, max_concurrent, budget, kGicpPairBytes, kGicpPointBytes);
}

// ghicp_gicp_clouds_trimmed: per pair the radix-select histograms of the ICP loop on top of that (its select record is within the 1024).
constexpr size_t kGicpTrimPairBytes = kGicpPairBytes + 6 * 2048 * 4;
inline std::vector<int> gh_gicp_trim_plan(int n_pairs, const int64_t* ns, int max_concurrent, size_t budget) {
  return gh_refine_plan(n_pairs, ns, max_concurrent, budget, kGicpTrimPairBytes, kGicpPointBytes);
}
