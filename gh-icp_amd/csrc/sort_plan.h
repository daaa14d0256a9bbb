// Host-side plan of the segmented radix sort (prims.hip): the one definition of the tile partition, and the digit places chosen from the
// key bits that are present.  Plain C++ (no HIP): tests/cpp/test_sort_plan.cpp builds it alone.
//   * A segment (a cloud of a launch sequence) is cut into tiles of GH_RS_TILE items; a tile never crosses a segment, so a segment's last
//     tile is partial and an empty segment has no tile.  Tiles are numbered through all segments (toff), and so are the chunks of
//     GH_RS_CHUNK tiles over which the per-digit counts are scanned (coff): a chunk never crosses a segment either.
//   * The significant bits are dealt evenly to the fewest places that digits of at most max_width bits allow.  9-bit digits are taken only
//     where they save a place against 8-bit ones (34 bits: 9 9 8 8 instead of five places; 24 bits stay 8 8 8).
#pragma once

constexpr int GH_RS_TILE = 4096;       // items per tile (256 threads x 16 items)
constexpr int GH_RS_CHUNK = 64;        // tiles per chunk
constexpr int GH_RS_MAX_SEGS = 64;     // segments per call (FB_MAX clouds of a launch sequence)
constexpr int GH_RS_MAX_WIDTH = 9;     // widest digit: 512 counters per wave as u16 keep the scatter's LDS at four workgroups per CU
constexpr int GH_RS_MAX_PLACES = 8;    // 64 bits in 8-bit digits

struct GhRsPlan {
  int places;
  int width[GH_RS_MAX_PLACES];  // bits of place p (place 0 = lowest bits); their sum is the bit count asked for
};

// bits in [0, 64]; max_width 8 or 9
inline GhRsPlan gh_rs_plan(int bits, int max_width = GH_RS_MAX_WIDTH) {
  GhRsPlan P;
  P.places = 0;
  for (int p = 0; p < GH_RS_MAX_PLACES; p++) P.width[p] = 0;
  if (bits <= 0) return P;
  const int p8 = (bits + 7) / 8, pw = (bits + max_width - 1) / max_width;
  P.places = pw < p8 ? pw : p8;
  const int base = bits / P.places, rem = bits % P.places;
  for (int p = 0; p < P.places; p++) P.width[p] = base + (p < rem ? 1 : 0);
  return P;
}

// The segments of one call, handed to every kernel of the sort by value (kernel arguments: scalar loads, no table in device memory)
struct GhRsSegs {
  int nseg;
  int off[GH_RS_MAX_SEGS + 1];   // items: segment s is [off[s], off[s + 1])
  int toff[GH_RS_MAX_SEGS + 1];  // tiles of the segments before s
  int coff[GH_RS_MAX_SEGS + 1];  // chunks of the segments before s
};

inline int gh_rs_tiles_of(long long n) { return (int)((n + GH_RS_TILE - 1) / GH_RS_TILE); }

// off: nseg + 1 ascending item offsets (off[0] is the first item of segment 0); returns the longest segment
template <typename T>
inline long long gh_rs_segs_make(GhRsSegs* S, int nseg, const T* off) {
  long long longest = 0;
  S->nseg = nseg;
  S->off[0] = (int)off[0]; S->toff[0] = 0; S->coff[0] = 0;
  for (int s = 0; s < nseg; s++) {
    const long long len = (long long)off[s + 1] - (long long)off[s];
    const int nt = gh_rs_tiles_of(len);
    S->off[s + 1] = (int)off[s + 1];
    S->toff[s + 1] = S->toff[s] + nt;
    S->coff[s + 1] = S->coff[s] + (nt + GH_RS_CHUNK - 1) / GH_RS_CHUNK;
    if (len > longest) longest = len;
  }
  for (int s = nseg + 1; s <= GH_RS_MAX_SEGS; s++) { S->off[s] = S->off[nseg]; S->toff[s] = S->toff[nseg]; S->coff[s] = S->coff[nseg]; }
  return longest;
}
