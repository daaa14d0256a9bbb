// Internal, host only (no HIP): how ghicp_clouds_prepare (prepare_clouds.hip) splits a list of clouds into chunks that share one launch
// sequence.  A chunk is a run of consecutive clouds of the list; it is closed when the next cloud would break one of the limits:
//   * PP_MAX_CLOUDS clouds (the descriptor tables of the kernels hold that many);
//   * the sum of points stays BELOW PP_MAX_POINTS (int indices into the concatenated cloud);
//   * per grid kind, the sum of cells stays at or below PP_MAX_CELLS (the sort key is cell base + cell in 32 bits, and the chunk's cell table
//     is one buffer of the context: 1 GB at the limit).  One cloud's grid holds at most 2^26 cells (gh_grid_desc), so a cloud always fits.
// A cloud that breaks a limit on its own still gets a chunk of its own: the callers never pass one (m < 2^31 - 2, cells <= 2^26).
// The same prefix rule picks, in every halving round of the fine cell, the clouds whose grids of that round fit one cell table together.
#pragma once
#include <cstdint>
#include <vector>

constexpr int PP_MAX_CLOUDS = 64;
constexpr long long PP_MAX_POINTS = (1ll << 31) - 2;
constexpr unsigned long long PP_MAX_CELLS = 1ull << 28;
constexpr int PP_KINDS = 3;  // grid kinds whose cells are known before the first launch: fine grid at its start cell, k-NN grid, overlap grid

struct PpSize {
  long long m;                          // points
  unsigned long long cells[PP_KINDS];   // cells per grid kind (0: the cloud does not need that grid)
};
struct PpLimits {
  int max_clouds = PP_MAX_CLOUDS;
  long long max_points = PP_MAX_POINTS;
  unsigned long long max_cells = PP_MAX_CELLS;
};
struct PpChunk { int first, count; };

// how many of sz[0 .. n) form the next chunk (>= 1 for n >= 1)
inline int pp_prefix(const PpSize* sz, int n, const PpLimits& L = PpLimits()) {
  long long pts = 0;
  unsigned long long cells[PP_KINDS] = {0, 0, 0};
  int i = 0;
  for (; i < n && i < L.max_clouds; i++) {
    bool fits = pts + sz[i].m < L.max_points;
    for (int k = 0; k < PP_KINDS; k++) fits = fits && cells[k] + sz[i].cells[k] <= L.max_cells;
    if (!fits) break;
    pts += sz[i].m;
    for (int k = 0; k < PP_KINDS; k++) cells[k] += sz[i].cells[k];
  }
  return (i == 0 && n > 0) ? 1 : i;
}

inline std::vector<PpChunk> pp_plan(const PpSize* sz, int n, const PpLimits& L = PpLimits()) {
  std::vector<PpChunk> out;
  for (int first = 0; first < n;) {
    const int c = pp_prefix(sz + first, n - first, L);
    out.push_back({first, c});
    first += c;
  }
  return out;
}
