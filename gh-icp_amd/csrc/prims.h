// Device-wide primitives of the front end, hand-written (prims.hip): inclusive scan, select-by-flag, unique over sorted keys.
// All enqueue on ctx->stream and return without synchronising; counts are written to device memory.
#pragma once
#include "ctx.h"
#include "sort_plan.h"

// data[i] = data[0] + ... + data[i], in place (u32, n <= 2^31)
int gh_scan_inclusive_u32(ghicp_ctx* ctx, unsigned* data, long long n);
// out_idx = the positions i (ascending) with flags[i] != 0; their number to d_count[0]   (was hipcub::DeviceSelect::Flagged over an iota)
int gh_select_flagged_iota(ghicp_ctx* ctx, const unsigned char* flags, long long n, int* out_idx, int* d_count);
// out = vals[i] for the positions i (ascending) with flags[i] != 0   (was hipcub::DeviceSelect::Flagged over a value array)
int gh_select_flagged_u32(ghicp_ctx* ctx, const unsigned* vals, const unsigned char* flags, long long n, unsigned* out, int* d_count);
// out = the distinct values of the SORTED array keys, ascending; their number to d_count[0]   (was hipcub::DeviceSelect::Unique)
int gh_unique_sorted_u32(ghicp_ctx* ctx, const unsigned* keys, long long n, unsigned* out, int* d_count);
// Stable radix sort on the key bits [bit_begin, bit_end), ascending; the input arrays are left untouched, the result is in keys_out / vals_out
// (vals_in == nullptr: keys only).  Spare buffer: B_GRID_TMP; table: B_PRIM_TMP.   (was rocprim::radix_sort_pairs / radix_sort_keys / hipcub::DeviceRadixSort)
int gh_radix_sort_u32(ghicp_ctx* ctx, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in, unsigned* vals_out, long long n, int bit_begin, int bit_end);
int gh_radix_sort_u64(ghicp_ctx* ctx, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* vals_in, unsigned* vals_out, long long n,
                      int bit_begin, int bit_end);
// The same sort segment by segment inside the same launches (the clouds of a launch sequence): segment s = items [off[s], off[s + 1]) of the arrays,
// off [host] = nseg + 1 ascending offsets from 0, nseg <= GH_RS_MAX_SEGS; segments may be empty.  Sorted on the bits [bit_begin, bit_begin + bits) of
// key - seg_base[s] (seg_base [device], nseg words, or nullptr for 0; every key of a segment >= its base): `bits` counts what the widest segment needs,
// not the segment's id.  Tiles, chunks and digit places: sort_plan.h.
// Two steps, so that the kernel that MAKES the keys can take the first place's counts on the way (the sort then skips its first histogram pass):
//   gh_rs_seg_begin   plans the sort (max_width: widest digit, 8 or 9; 0: ctx->sort_digit_bits) and reserves its table.  R->first.table != nullptr: a
//                     key-making kernel launched over R->S's tiles (one workgroup of 256 threads per tile, gh_rs_tile) may leave the tile's counts of
//                     the digit (key - base) >> bit_begin & R->first.mask there with gh_rs_first_*, and then sets R->have_first.
//   gh_radix_sort_seg_*  runs the places.  Nothing else may use B_PRIM_TMP between the two.
struct GhRsFirst {
  unsigned* table;  // table[tile][nd]; nullptr: no counts wanted (no place, or no segment beyond one tile: all places in one launch)
  int nd;           // digits of the first place's table row: 256 or 512
  unsigned mask;
};
struct GhRsSort {
  GhRsSegs S;
  GhRsPlan P;
  long long longest;
  GhRsFirst first;
  bool have_first;
};
int gh_rs_seg_begin(ghicp_ctx* ctx, int nseg, const int* off, int bits, int max_width, GhRsSort* R);
int gh_radix_sort_seg_u32(ghicp_ctx* ctx, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in, unsigned* vals_out, const GhRsSort& R,
                          const unsigned* seg_base, int bit_begin);
int gh_radix_sort_seg_u64(ghicp_ctx* ctx, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* vals_in, unsigned* vals_out,
                          const GhRsSort& R, int bit_begin);

// ---- device side of the tile partition (the sort's kernels and the key-making kernels of batch.hip share it)
__device__ inline int gh_rs_find(const int* off, int nseg, int i) {  // largest s in [0, nseg) with off[s] <= i: empty segments are skipped over
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
struct GhRsTile { int seg, first, here; };  // a tile's segment, its first item, its items
__device__ inline GhRsTile gh_rs_tile(const GhRsSegs& S, int g) {
  GhRsTile t;
  t.seg = gh_rs_find(S.toff, S.nseg, g);
  t.first = S.off[t.seg] + (g - S.toff[t.seg]) * GH_RS_TILE;
  const int left = S.off[t.seg + 1] - t.first;
  t.here = left < GH_RS_TILE ? left : GH_RS_TILE;
  return t;
}
// The first place's counts of a tile, taken by the 256-thread workgroup that makes the tile's keys: cnt is LDS, one row per wave.
constexpr int GH_RS_MAX_ND = 1 << GH_RS_MAX_WIDTH;
__device__ inline void gh_rs_first_zero(unsigned (*cnt)[GH_RS_MAX_ND], int nd) {
  for (int w = 0; w < 4; w++)
    for (int d = threadIdx.x; d < nd; d += 256) cnt[w][d] = 0u;
  __syncthreads();
}
__device__ inline void gh_rs_first_add(unsigned (*cnt)[GH_RS_MAX_ND], unsigned digit) { atomicAdd(&cnt[threadIdx.x >> 6][digit], 1u); }
__device__ inline void gh_rs_first_store(unsigned (*cnt)[GH_RS_MAX_ND], const GhRsFirst& F, int tile) {
  __syncthreads();
  for (int d = threadIdx.x; d < F.nd; d += 256) F.table[(size_t)tile * F.nd + d] = cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d];
}
