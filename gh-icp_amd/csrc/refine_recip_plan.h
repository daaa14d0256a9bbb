// Internal: the two pieces of arithmetic behind the per-iteration source grids of ghicp_refine_clouds_reciprocal (refine_recip.hip) -- the cell
// budget of every pair of a chunk (host, once per chunk) and the grid a pair gets inside its budget (device, once per pair per iteration).
// Plain C++ without HIP types: tests/cpp/test_refine_recip_plan.cpp compiles both on their own.
//
// Budget rule.  The cell table of a chunk is reserved before the loop, so a pair cannot be given the cells its moved source would like in
// some iteration: it gets a FIXED range of the table -- kRecipFineCells cells per source point (+ kRecipMinCells) for its fine grid and
// kRecipCoarseCells per point (+ kRecipMinCells) for its coarse grid; the fine ranges of the chunk's pairs come first, in pair order, then the
// coarse ranges, each base the prefix sum of the ranges before it.  64 cells per point is what a surface scan at the target's fine cell
// (chosen by ghicp_icp for <= 8 points per OCCUPIED cell) typically spreads over; gh_refine_plan pays 4 B per cell through kRecipPointBytes
// (refine_plan.h).  A chunk whose ranges would exceed kRecipMaxCells (keys are 32 bits; a caller may force any chunk size) halves the
// per-point multiples until they fit: a larger cell is still exact.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_RECIP_HD __host__ __device__
#else
#define GH_RECIP_HD
#endif

constexpr unsigned kRecipFineCells = 64;    // cells per source point of a pair's fine range
constexpr unsigned kRecipCoarseCells = 1;   // ... of its coarse range (the coarse cell is 8 x the fine one: 512 x fewer cells over the same box)
constexpr unsigned kRecipMinCells = 64;     // added to every range: a pair of three points still gets a grid
constexpr unsigned long long kRecipMaxCells = 1ull << 30;  // cells of one chunk's table, fine and coarse ranges together

struct RecipRange {
  unsigned base_f, cells_f;  // the pair's fine range of the chunk's cell table: [base_f, base_f + cells_f)
  unsigned base_c, cells_c;  // its coarse range (bases count from the start of the table: the coarse ranges follow the last fine range)
};

// Ranges of the np pairs of a chunk (ns[p]: source points, <= 0 for a pair that never runs: it gets the minimum).  Returns the cells of the
// whole table: the host reserves exactly that many (+ the closing entry).
inline unsigned long long gh_recip_ranges(int np, const int* ns, RecipRange* out) {
  unsigned long long pts = 0;
  for (int p = 0; p < np; p++) pts += (unsigned long long)(ns[p] > 0 ? ns[p] : 0);
  unsigned shift = 0;  // both multiples are divided by 2^shift
  while (shift < 32 && ((pts * kRecipFineCells) >> shift) + ((pts * kRecipCoarseCells) >> shift) + 2ull * kRecipMinCells * (unsigned long long)np > kRecipMaxCells) shift++;
  unsigned long long at = 0;
  for (int p = 0; p < np; p++) {
    const unsigned long long n = (unsigned long long)(ns[p] > 0 ? ns[p] : 0);
    out[p].base_f = (unsigned)at;
    out[p].cells_f = (unsigned)(shift < 32 ? (n * kRecipFineCells) >> shift : 0ull) + kRecipMinCells;
    at += out[p].cells_f;
  }
  for (int p = 0; p < np; p++) {
    const unsigned long long n = (unsigned long long)(ns[p] > 0 ? ns[p] : 0);
    out[p].base_c = (unsigned)at;
    out[p].cells_c = (unsigned)(shift < 32 ? (n * kRecipCoarseCells) >> shift : 0ull) + kRecipMinCells;
    at += out[p].cells_c;
  }
  return at;
}

struct RecipGrid {  // the fields of GridDesc (grid.h) a search needs
  float mn[3];
  float inv;
  int dim[3];
  unsigned ncell;
};

// The grid over the box mm[0..2] .. mm[3..5] with a cell of at least `cell` and at most `budget` (>= 1) cells: gh_grid_desc's rule (the cell
// widened with the extent beyond 256 cells per axis, then multiplied by 1.5 until the table fits), with the pair's budget in place of the
// 2^26 cells of a grid that owns its table.  A box that is not finite, or that nothing coarsens into the budget, ends as ONE cell: every
// point is clamped into it (gh_cell_coord) and the search stays exact.
GH_RECIP_HD inline RecipGrid gh_recip_grid(const float* mm, float cell, unsigned budget) {
  RecipGrid g;
  float ext = 0.f;
  for (int d = 0; d < 3; d++) {
    g.mn[d] = mm[d];
    const float e = mm[3 + d] - mm[d];
    ext = ext > e ? ext : e;
  }
  const float dims = ext / cell;
  if (dims > 256.f) cell *= 1.0f + 4e-7f * dims;
  for (int it = 0; it < 256; it++) {
    g.inv = 1.0f / cell;
    unsigned long long nc = 1;
    bool fits = true;
    for (int d = 0; d < 3; d++) {
      const float f = floorf((mm[3 + d] - mm[d]) * g.inv);
      if (!(f < 1.0e9f)) { fits = false; break; }  // (also a NaN)
      g.dim[d] = f < 0.f ? 1 : (int)f + 1;
      nc *= (unsigned long long)g.dim[d];
      if (nc > (unsigned long long)budget) { fits = false; break; }
    }
    if (fits) { g.ncell = (unsigned)nc; return g; }
    cell *= 1.5f;
  }
  g.inv = 1.0f / cell;
  g.dim[0] = g.dim[1] = g.dim[2] = 1;
  g.ncell = 1;
  return g;
}

// cell coordinate of v on one axis: gh_cell_coord (grid.h) restated for the host check (the clamp before the conversion: the device's
// float -> int conversion saturates, the host's is undefined out of range)
GH_RECIP_HD inline int gh_recip_coord(float v, float mn, float inv, int dim) {
  const float f = floorf((v - mn) * inv);
  if (!(f > 0.f)) return 0;
  return f >= (float)(dim - 1) ? dim - 1 : (int)f;
}
