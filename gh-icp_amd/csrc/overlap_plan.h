// Internal: how ghicp_overlap_clouds (overlap_clouds.hip) cuts its pairs into chunks -- the pairs of ONE launch -- and how a block of that launch
// finds its pair.  A chunk's blocks are the concatenation of cdiv(ns[p], 256) blocks per pair on a 1-D grid: no block spans two pairs, and a chunk
// whose sources differ a lot in size launches no surplus blocks.  Plain C++, no HIP include: compiled on its own by tests/cpp/test_overlap_plan.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GH_OV_HD __host__ __device__
#else
#define GH_OV_HD
#endif

constexpr int kOvBlock = 256;                  // threads per block = source points per block
constexpr int kOvMaxChunk = 4096;              // pairs per launch at most (max_concurrent = 0, or larger values)
constexpr long long kOvMaxBlocks = 1ll << 24;  // blocks per launch a chunk is cut at (a single larger pair still gets a chunk of its own)

struct OvChunk {
  int p0 = 0, p1 = 0;      // the pairs [p0, p1) of the call
  std::vector<int> first;  // p1 - p0 + 1 entries: first[q] = first block of pair p0 + q, first.back() = blocks of the launch
};

inline long long gh_ov_blocks(int64_t ns) { return ns > 0 ? (long long)((ns + kOvBlock - 1) / kOvBlock) : 0; }

// The chunks of n_pairs pairs in the given order; ns[p]: the source points pair p launches (0: a pair with an empty side -- it belongs to a chunk
// and owns no block).  max_concurrent > 0: chunks of exactly that many pairs (the last one shorter), capped at kOvMaxChunk; 0: kOvMaxChunk.
// Either way a chunk ends before the pair that would take it past max_blocks blocks, unless it is the chunk's first pair.  Empty list: no chunk.
inline std::vector<OvChunk> gh_overlap_plan(int n_pairs, const int64_t* ns, int max_concurrent, long long max_blocks = kOvMaxBlocks) {
  std::vector<OvChunk> plan;
  if (n_pairs <= 0) return plan;
  const int cap = max_concurrent > 0 && max_concurrent < kOvMaxChunk ? max_concurrent : kOvMaxChunk;
  OvChunk cur;
  cur.first.push_back(0);
  for (int p = 0; p < n_pairs; p++) {
    const long long nb = gh_ov_blocks(ns[p]);
    const int in_chunk = p - cur.p0;
    if (in_chunk >= cap || (in_chunk > 0 && (long long)cur.first.back() + nb > max_blocks)) {
      cur.p1 = p;
      plan.push_back(cur);
      cur = OvChunk();
      cur.p0 = p;
      cur.first.push_back(0);
    }
    cur.first.push_back((int)((long long)cur.first.back() + nb));
  }
  cur.p1 = n_pairs;
  plan.push_back(cur);
  return plan;
}

// The pair (index within the chunk) that owns block b, 0 <= b < first[np]: the LAST q < np with first[q] <= b.  A pair without blocks has
// first[q] == first[q + 1], so whenever it satisfies the test its successor does too: it is never returned.
GH_OV_HD inline int gh_ov_pair_of_block(const int* first, int np, int b) {
  int lo = 0, hi = np - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
