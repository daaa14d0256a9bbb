// Hand-written device-wide primitives of the front end (gfx950): inclusive scan, select-by-flag and unique over a sorted run
// (round-5 verdict, missing #3 / next-round item 5: these were hipcub::DeviceSelect / rocPRIM calls -- two launches each plus a
// temporary-storage query, a look-back state kernel and runtime fill kernels in every profile).
// All three are the same three launches over tiles of TILE items per 256-thread workgroup:
//   (1) tile totals                     -- one pass over the input, wave ballots / DPP adds, one number per tile
//   (2) scan of the tile totals         -- a single workgroup (<= 2^28 / TILE = 64 K totals)
//   (3) tile-local scan + tile offset   -- second pass over the input, outputs written in order (stable, ascending)
// Reading the input twice costs less than the host round trips and look-back spinning it replaces at these sizes (1-60 M items, HBM
// bound either way), and the result is position-exact: item i of the output is the i-th flagged / distinct input.
#include "prims.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace {

constexpr int PT = 256;           // threads per workgroup
constexpr int PI = 16;            // items per thread
constexpr int TILE = PT * PI;     // 4096 items per tile

__device__ inline unsigned wave_incl_scan(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// exclusive prefix of `v` over the workgroup (sh: 4 words); returns the prefix, *total = workgroup sum
__device__ inline unsigned block_excl_scan(unsigned v, unsigned* sh, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned inc = wave_incl_scan(v, lane);
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  unsigned base = 0;
  for (int w = 0; w < wave; w++) base += sh[w];
  *total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return base + inc - v;
}

// ---- (1) tile totals.  MODE 0: sum of u32 values; 1: number of non-zero flag bytes; 2: number of run heads of a sorted u32 array
template <int MODE>
__global__ __launch_bounds__(PT) void k_tile_totals(const void* __restrict__ in, long long n, unsigned* __restrict__ totals) {
  __shared__ unsigned sh[4];
  const long long t0 = (long long)blockIdx.x * TILE;
  unsigned acc = 0;
#pragma unroll 4
  for (int k = 0; k < PI; k++) {
    const long long i = t0 + (long long)k * PT + threadIdx.x;
    if (i < n) {
      if (MODE == 0) acc += reinterpret_cast<const unsigned*>(in)[i];
      else if (MODE == 1) acc += reinterpret_cast<const unsigned char*>(in)[i] ? 1u : 0u;
      else {
        const unsigned* key = reinterpret_cast<const unsigned*>(in);
        acc += (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
      }
    }
  }
  unsigned tot;
  block_excl_scan(acc, sh, &tot);
  if (threadIdx.x == 0) totals[blockIdx.x] = tot;
}

// ---- (2) exclusive scan of the tile totals in place, one workgroup; totals[nt] = grand total (also to *count when given)
__global__ __launch_bounds__(PT) void k_scan_totals(unsigned* __restrict__ totals, int nt, int* __restrict__ count) {
  __shared__ unsigned sh[4];
  unsigned carry = 0;
  for (int base = 0; base < nt; base += PT) {
    const int i = base + threadIdx.x;
    const unsigned v = i < nt ? totals[i] : 0u;
    unsigned tot;
    const unsigned ex = block_excl_scan(v, sh, &tot);
    if (i < nt) totals[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    totals[nt] = carry;
    if (count) *count = (int)carry;
  }
}

// ---- (3a) inclusive scan in place.  A thread owns PI CONSECUTIVE items so that one prefix per thread suffices.
__global__ __launch_bounds__(PT) void k_scan_apply(unsigned* __restrict__ data, long long n, const unsigned* __restrict__ totals) {
  __shared__ unsigned sh[4];
  const long long t0 = (long long)blockIdx.x * TILE + (long long)threadIdx.x * PI;
  unsigned v[PI];
  unsigned acc = 0;
  // 64 bytes per thread as four 16-byte accesses -- only when the thread's range lies inside n AND starts on a 16-byte boundary: t0 is a multiple
  // of 16 items, so that is a property of `data` alone (uniform over the launch).  A base that is merely 4-byte aligned (batch_nms.hip scans
  // `table + 1`) takes the item-wise path, like the thread that straddles n.
  const bool whole = t0 + PI <= n && (reinterpret_cast<uintptr_t>(data) & 15u) == 0;
  if (whole) {
#pragma unroll
    for (int q = 0; q < PI / 4; q++) {
      const uint4 u = reinterpret_cast<const uint4*>(data + t0)[q];
      v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PI; k++) v[k] = t0 + k < n ? data[t0 + k] : 0u;
  }
#pragma unroll
  for (int k = 0; k < PI; k++) acc += v[k];
  unsigned tot;
  unsigned run = totals[blockIdx.x] + block_excl_scan(acc, sh, &tot);
#pragma unroll
  for (int k = 0; k < PI; k++) {
    run += v[k];
    v[k] = run;
  }
  if (whole) {
#pragma unroll
    for (int q = 0; q < PI / 4; q++) reinterpret_cast<uint4*>(data + t0)[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < PI; k++)
      if (t0 + k < n) data[t0 + k] = v[k];
  }
}

// ---- (3b) select: out[rank] = i for every flagged (MODE 1) / run-head (MODE 2) position i, ascending; MODE 2 writes the KEY instead
// (unique).  Items are taken wave-contiguously (a wave instruction covers 64 consecutive items), ranks from ballots.
template <int MODE>
__global__ __launch_bounds__(PT) void k_select_apply(const void* __restrict__ in, long long n, const unsigned* __restrict__ totals, unsigned* __restrict__ out,
                                                     const unsigned* __restrict__ vals) {
  __shared__ unsigned sh_w[4][PI];  // per wave and round: hits of that wave in that round
  __shared__ unsigned sh_base[4][PI];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long t0 = (long long)blockIdx.x * TILE;
  // item (round k, wave w, lane l) = t0 + (k * 4 + w) * 64 + l: ascending in (k, w, l)
  unsigned long long hit[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const long long i = t0 + (long long)(k * 4 + wave) * 64 + lane;
    bool h = false;
    if (i < n) {
      if (MODE == 1) h = reinterpret_cast<const unsigned char*>(in)[i] != 0;
      else {
        const unsigned* key = reinterpret_cast<const unsigned*>(in);
        h = i == 0 || key[i] != key[i - 1];
      }
    }
    hit[k] = __ballot(h);
    if (lane == 0) sh_w[wave][k] = (unsigned)__popcll(hit[k]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // 64 numbers: serial prefix in (k, w) order
    unsigned run = totals[blockIdx.x];
    for (int k = 0; k < PI; k++)
      for (int w = 0; w < 4; w++) { sh_base[w][k] = run; run += sh_w[w][k]; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PI; k++) {
    if ((hit[k] >> lane) & 1ull) {
      const long long i = t0 + (long long)(k * 4 + wave) * 64 + lane;
      const unsigned pos = sh_base[wave][k] + (unsigned)__popcll(hit[k] & ((1ull << lane) - 1ull));
      out[pos] = MODE == 1 ? (vals ? vals[i] : (unsigned)i) : reinterpret_cast<const unsigned*>(in)[i];
    }
  }
}

int tiles_of(long long n) { return (int)((n + TILE - 1) / TILE); }

// ================================================================================ stable LSD radix sort (round 6)
// Replaces rocPRIM's Onesweep for the voxel keys, the two grids' cell keys and the single-cloud NMS order (filter.hpp:66,
// keypoint_detect.hpp:119-130: the reference's std::sort calls; stability = "lowest input index leads its voxel / cell").
// One pass per 8-bit digit place, four launches per pass over the same 4096-item tiles as the scan / select above:
//   k_rs_hist     digit counts of every tile                      -> table[tile][digit]   (1 KB per tile, written coalesced)
//   k_rs_chunks   per digit, exclusive scan over a chunk of tiles -> table (in place), chunk totals part[chunk][digit]
//   k_rs_bases    one workgroup: chunk totals -> chunk bases per digit, digit totals -> digit bases
//   k_rs_scatter  ranks inside the tile from wave ballots (items in input order: wave-contiguous chunks, a wave's rounds in turn), the
//                 tile reordered by digit in LDS, then written out as runs -- consecutive threads store consecutive addresses of a run
// (three launches per place up to 64 tiles: k_rs_chunk_bases, and up to 32 chunks = 8 M items: the scatter sums the chunk rows itself; ONE launch for all
// places up to one tile: k_rs_small)
// No look-back, no spinning, no temporary-storage query; position-exact, so the result does not depend on the launch order of workgroups.
constexpr int RD = 256;   // digits per place
constexpr int RC = 64;    // tiles per chunk of k_rs_chunks

template <typename K>
__global__ __launch_bounds__(PT) void k_rs_hist(const K* __restrict__ keys, long long n, int shift, unsigned mask, unsigned* __restrict__ table) {
  __shared__ unsigned cnt[4][RD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < 4; w++) cnt[w][threadIdx.x] = 0u;
  __syncthreads();
  const long long t0 = (long long)blockIdx.x * TILE;
  K key[PI];  // all loads of the tile in flight before the first LDS atomic
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const long long i = t0 + (long long)(wave * PI + k) * 64 + lane;
    key[k] = i < n ? keys[i] : (K)0;
  }
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const long long i = t0 + (long long)(wave * PI + k) * 64 + lane;
    if (i < n) atomicAdd(&cnt[wave][(unsigned)(key[k] >> shift) & mask], 1u);
  }
  __syncthreads();
  table[(size_t)blockIdx.x * RD + threadIdx.x] = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
}

// thread = digit; a workgroup walks RC consecutive tiles (rows of 1 KB, coalesced)
__global__ __launch_bounds__(RD) void k_rs_chunks(unsigned* __restrict__ table, int nt, unsigned* __restrict__ part) {
  const int t0 = blockIdx.x * RC, t1 = t0 + RC < nt ? t0 + RC : nt;
  unsigned run = 0;
#pragma unroll 8
  for (int t = t0; t < t1; t++) {
    const unsigned v = table[(size_t)t * RD + threadIdx.x];
    table[(size_t)t * RD + threadIdx.x] = run;
    run += v;
  }
  part[(size_t)blockIdx.x * RD + threadIdx.x] = run;
}

__global__ __launch_bounds__(RD) void k_rs_bases(unsigned* __restrict__ part, int nchunk, unsigned* __restrict__ digit_base) {
  __shared__ unsigned sh[4];
  unsigned run = 0;
#pragma unroll 8
  for (int j = 0; j < nchunk; j++) {
    const unsigned v = part[(size_t)j * RD + threadIdx.x];
    part[(size_t)j * RD + threadIdx.x] = run;
    run += v;
  }
  unsigned tot;
  digit_base[threadIdx.x] = block_excl_scan(run, sh, &tot);
}

// One digit place of one tile, by the whole workgroup: the items (key[k], val[k] of item (wave * PI + k) * 64 + lane, `here` of them) end up in
// T.lk / T.lv in stable order of the digit, T.first[d] = first position of digit d.  Ranks from wave ballots: a wave owns PI * 64 consecutive
// items and takes them 64 at a time; the lanes of a round that share a digit find each other with eight ballots, the lowest of them bumps the
// wave's counter of that digit (LDS, that one lane only) and hands the old value round.  Ends with a barrier.
// ND digits per place: 256, or 512 for the 9-bit places of the segmented sort (sort_plan.h).  No count exceeds the tile's 4096 items, so the 512
// counters are u16: the tile stays at 39 KB of LDS, four workgroups to a CU as with 256.  `kbase` is taken off the key before the digit (the
// segmented sort of global cell keys; 0 elsewhere).
template <typename K, bool HASV, int ND = 256>
struct RsTile {
  typedef typename std::conditional<(ND > 256), unsigned short, unsigned>::type C;
  C cnt[4][ND];  // per wave: running count of a digit, then the wave's base inside the digit's run of this tile
  C first[ND];
  unsigned sh[4];
  K lk[TILE];
  unsigned lv[HASV ? TILE : 1];
};
template <typename K, bool HASV, int ND = 256>
__device__ inline void rs_tile_sort(RsTile<K, HASV, ND>& T, const K (&key)[PI], const unsigned (&val)[PI], int here, int shift, unsigned mask, K kbase = (K)0) {
  constexpr int DPT = ND / PT;  // digits per thread where thread = digit: DPT consecutive ones
  constexpr int NB = ND > 256 ? 9 : 8;
  typedef typename RsTile<K, HASV, ND>::C C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < 4; w++)
#pragma unroll
    for (int q = 0; q < DPT; q++) T.cnt[w][q * PT + threadIdx.x] = (C)0;
  __syncthreads();
  unsigned rk[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const bool valid = (wave * PI + k) * 64 + lane < here;
    const unsigned d = (unsigned)((key[k] - kbase) >> shift) & mask;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < NB; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int leader = valid ? (int)__ffsll(peers) - 1 : lane;
    unsigned base = 0;
    if (valid && lane == leader) {
      base = T.cnt[wave][d];
      T.cnt[wave][d] = (C)(base + (unsigned)__popcll(peers));
    }
    base = __shfl(base, leader, 64);
    rk[k] = base + (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  {  // thread = digit: the waves' bases inside the digit's run, the run's place in the tile
    unsigned sum[DPT], all = 0;
#pragma unroll
    for (int q = 0; q < DPT; q++) {
      const int d = threadIdx.x * DPT + q;
      const unsigned c0 = T.cnt[0][d], c1 = T.cnt[1][d], c2 = T.cnt[2][d], c3 = T.cnt[3][d];
      T.cnt[0][d] = (C)0; T.cnt[1][d] = (C)c0; T.cnt[2][d] = (C)(c0 + c1); T.cnt[3][d] = (C)(c0 + c1 + c2);
      sum[q] = c0 + c1 + c2 + c3;
      all += sum[q];
    }
    unsigned tot;
    unsigned run = block_excl_scan(all, T.sh, &tot);
#pragma unroll
    for (int q = 0; q < DPT; q++) {
      T.first[threadIdx.x * DPT + q] = (C)run;
      run += sum[q];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PI; k++) {
    if ((wave * PI + k) * 64 + lane < here) {
      const unsigned d = (unsigned)((key[k] - kbase) >> shift) & mask;
      const unsigned p = (unsigned)T.first[d] + (unsigned)T.cnt[wave][d] + rk[k];
      T.lk[p] = key[k];
      if (HASV) T.lv[p] = val[k];
    }
  }
  __syncthreads();
}

// BASES: the launch has no k_rs_bases before it (up to RS_INLINE_CHUNKS chunks): `part` holds the chunks' raw totals and every workgroup sums the
// few rows it needs itself (thread = digit; the rows come out of L2) -- a launch less per digit place where launches are what a place costs.
constexpr int RS_INLINE_CHUNKS = 32;
template <typename K, bool HASV, bool BASES>
__global__ __launch_bounds__(PT) void k_rs_scatter(const K* __restrict__ kin, const unsigned* __restrict__ vin, K* __restrict__ kout, unsigned* __restrict__ vout,
                                                   long long n, int shift, unsigned mask, const unsigned* __restrict__ table, const unsigned* __restrict__ part,
                                                   const unsigned* __restrict__ digit_base, int nchunk) {
  __shared__ RsTile<K, HASV> T;
  __shared__ unsigned s_delta[RD];  // global position of the digit's run of this tile - its first position in the tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long t0 = (long long)blockIdx.x * TILE;
  const int here = n - t0 < (long long)TILE ? (int)(n - t0) : TILE;
  K key[PI];
  unsigned val[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const long long i = t0 + (long long)(wave * PI + k) * 64 + lane;
    key[k] = i < n ? kin[i] : (K)0;
    val[k] = (HASV && i < n) ? vin[i] : 0u;
  }
  unsigned run_at = table[(size_t)blockIdx.x * RD + threadIdx.x];  // thread = digit
  if (BASES) {
    const int mine = (int)blockIdx.x / RC;
    unsigned below = 0, total = 0;
    for (int j = 0; j < nchunk; j++) {
      const unsigned v = part[(size_t)j * RD + threadIdx.x];
      total += v;
      below += j < mine ? v : 0u;
    }
    unsigned tot;
    run_at += below + block_excl_scan(total, T.sh, &tot);
  } else {
    run_at += digit_base[threadIdx.x] + part[(size_t)(blockIdx.x / RC) * RD + threadIdx.x];
  }
  rs_tile_sort<K, HASV>(T, key, val, here, shift, mask);
  s_delta[threadIdx.x] = run_at - T.first[threadIdx.x];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PI; j++) {
    const int p = j * PT + threadIdx.x;
    if (p < here) {
      const K kk = T.lk[p];
      const unsigned pos = s_delta[(unsigned)(kk >> shift) & mask] + (unsigned)p;
      kout[pos] = kk;
      if (HASV) vout[pos] = T.lv[p];
    }
  }
}

// n <= TILE: every digit place in ONE launch of one workgroup (the single-cloud front end's NMS order, small grids): the items stay in
// registers between the places and go through the tile once per place.
template <typename K, bool HASV>
__global__ __launch_bounds__(PT) void k_rs_small(const K* __restrict__ kin, const unsigned* __restrict__ vin, K* __restrict__ kout, unsigned* __restrict__ vout, int n,
                                                 int bit_begin, int bit_end) {
  __shared__ RsTile<K, HASV> T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  K key[PI];
  unsigned val[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const int i = (wave * PI + k) * 64 + lane;
    key[k] = i < n ? kin[i] : (K)0;
    val[k] = (HASV && i < n) ? vin[i] : 0u;
  }
  for (int shift = bit_begin; shift < bit_end; shift += 8) {
    const unsigned mask = (1u << (bit_end - shift < 8 ? bit_end - shift : 8)) - 1u;
    rs_tile_sort<K, HASV>(T, key, val, n, shift, mask);
    if (shift + 8 < bit_end) {
#pragma unroll
      for (int k = 0; k < PI; k++) {
        const int i = (wave * PI + k) * 64 + lane;
        if (i < n) {
          key[k] = T.lk[i];
          if (HASV) val[k] = T.lv[i];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PI; j++) {
    const int p = j * PT + threadIdx.x;
    if (p < n) {
      kout[p] = T.lk[p];
      if (HASV) vout[p] = T.lv[p];
    }
  }
}

// nt <= RC: k_rs_chunks and k_rs_bases in one launch (one chunk: its base is 0)
__global__ __launch_bounds__(RD) void k_rs_chunk_bases(unsigned* __restrict__ table, int nt, unsigned* __restrict__ part, unsigned* __restrict__ digit_base) {
  __shared__ unsigned sh[4];
  unsigned run = 0;
#pragma unroll 8
  for (int t = 0; t < nt; t++) {
    const unsigned v = table[(size_t)t * RD + threadIdx.x];
    table[(size_t)t * RD + threadIdx.x] = run;
    run += v;
  }
  part[threadIdx.x] = 0u;
  unsigned tot;
  digit_base[threadIdx.x] = block_excl_scan(run, sh, &tot);
}

template <typename K>
int radix_sort_impl(ghicp_ctx* ctx, const K* kin, K* kout, const unsigned* vin, unsigned* vout, long long n, int bit_begin, int bit_end) {
  if (n <= 0) return GHICP_OK;
  hipStream_t s = ctx->stream;
  const bool hasv = vin != nullptr;
  const int passes = bit_end > bit_begin ? (bit_end - bit_begin + 7) / 8 : 0;
  if (passes == 0) {
    GH_HIP(hipMemcpyAsync(kout, kin, (size_t)n * sizeof(K), hipMemcpyDeviceToDevice, s));
    if (hasv) GH_HIP(hipMemcpyAsync(vout, vin, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    return GHICP_OK;
  }
  if (n <= TILE) {
    if (hasv) hipLaunchKernelGGL((k_rs_small<K, true>), dim3(1), dim3(PT), 0, s, kin, vin, kout, vout, (int)n, bit_begin, bit_end);
    else hipLaunchKernelGGL((k_rs_small<K, false>), dim3(1), dim3(PT), 0, s, kin, (const unsigned*)nullptr, kout, (unsigned*)nullptr, (int)n, bit_begin, bit_end);
    GH_HIP(hipGetLastError());
    return GHICP_OK;
  }
  const int nt = tiles_of(n), nchunk = (nt + RC - 1) / RC;
  unsigned* table;
  GH_TRY(ctx->reserve(B_PRIM_TMP, (size_t)nt * RD + (size_t)nchunk * RD + RD + 4, &table));
  unsigned* part = table + (size_t)nt * RD;
  unsigned* digit_base = part + (size_t)nchunk * RD;
  // the input is left alone: passes alternate between a spare buffer and the output so that the last one lands in the output
  K* spare_k = nullptr;
  unsigned* spare_v = nullptr;
  if (passes > 1) {
    char* sp;
    const size_t kb = (((size_t)n * sizeof(K) + 255) / 256) * 256;
    GH_TRY(ctx->reserve(B_GRID_TMP, kb + (hasv ? (size_t)n * sizeof(unsigned) : 0) + 16, &sp));
    spare_k = reinterpret_cast<K*>(sp);
    spare_v = reinterpret_cast<unsigned*>(sp + kb);
  }
  const K* src_k = kin;
  const unsigned* src_v = vin;
  for (int p = 0; p < passes; p++) {
    const bool to_out = ((passes - 1 - p) & 1) == 0;
    K* dst_k = to_out ? kout : spare_k;
    unsigned* dst_v = to_out ? vout : spare_v;
    const int shift = bit_begin + 8 * p;
    const unsigned mask = (1u << std::min(8, bit_end - shift)) - 1u;
    hipLaunchKernelGGL((k_rs_hist<K>), dim3(nt), dim3(PT), 0, s, src_k, n, shift, mask, table);
    const bool inline_bases = nchunk > 1 && nchunk <= RS_INLINE_CHUNKS;
    if (nchunk == 1) hipLaunchKernelGGL(k_rs_chunk_bases, dim3(1), dim3(RD), 0, s, table, nt, part, digit_base);
    else {
      hipLaunchKernelGGL(k_rs_chunks, dim3(nchunk), dim3(RD), 0, s, table, nt, part);
      if (!inline_bases) hipLaunchKernelGGL(k_rs_bases, dim3(1), dim3(RD), 0, s, part, nchunk, digit_base);
    }
    const unsigned* tb = table;
    const unsigned* pt = part;
    const unsigned* db = digit_base;
    const unsigned* nov = nullptr;
    unsigned* novo = nullptr;
    if (hasv && inline_bases) hipLaunchKernelGGL((k_rs_scatter<K, true, true>), dim3(nt), dim3(PT), 0, s, src_k, src_v, dst_k, dst_v, n, shift, mask, tb, pt, db, nchunk);
    else if (hasv) hipLaunchKernelGGL((k_rs_scatter<K, true, false>), dim3(nt), dim3(PT), 0, s, src_k, src_v, dst_k, dst_v, n, shift, mask, tb, pt, db, nchunk);
    else if (inline_bases) hipLaunchKernelGGL((k_rs_scatter<K, false, true>), dim3(nt), dim3(PT), 0, s, src_k, nov, dst_k, novo, n, shift, mask, tb, pt, db, nchunk);
    else hipLaunchKernelGGL((k_rs_scatter<K, false, false>), dim3(nt), dim3(PT), 0, s, src_k, nov, dst_k, novo, n, shift, mask, tb, pt, db, nchunk);
    src_k = dst_k;
    src_v = dst_v;
  }
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

// ================================================================================ segmented places (sort_plan.h)
// The clouds of a launch sequence sorted cloud by cloud inside the same launches: a tile lies in one segment, the counts are kept per (segment,
// place, tile) and scanned per segment, so the segment's id is not among the sorted bits -- 34 instead of 39 bits for the packed voxel keys of 32
// clouds, and digits of up to 9 bits make that four places.  The segments travel as a kernel argument (GhRsSegs): a workgroup finds its tile's
// segment with a binary search over scalar loads.  Launches per place: k_rss_hist, k_rss_chunks, k_rss_bases, k_rss_scatter; three when no segment
// has more than one chunk (k_rss_bases walks the tiles itself); ONE for all places when no segment has more than one tile (k_rss_small).
static_assert(TILE == GH_RS_TILE && RC == GH_RS_CHUNK, "sort_plan.h defines the tile partition");

// (gh_rs_find / gh_rs_tile: prims.h, shared with the kernels that make the keys and may leave the first place's counts: GhRsFirst)

template <typename K, int ND>
__global__ __launch_bounds__(PT) void k_rss_hist(const K* __restrict__ keys, GhRsSegs S, const unsigned* __restrict__ kbase, int shift, unsigned mask,
                                                 unsigned* __restrict__ table) {
  __shared__ unsigned cnt[4][ND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < 4; w++)
#pragma unroll
    for (int q = 0; q < ND / PT; q++) cnt[w][q * PT + threadIdx.x] = 0u;
  __syncthreads();
  const GhRsTile t = gh_rs_tile(S, (int)blockIdx.x);
  const K kb = kbase ? (K)kbase[t.seg] : (K)0;
  K key[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const int j = (wave * PI + k) * 64 + lane;
    key[k] = j < t.here ? keys[(size_t)t.first + j] : (K)0;
  }
#pragma unroll
  for (int k = 0; k < PI; k++)
    if ((wave * PI + k) * 64 + lane < t.here) atomicAdd(&cnt[wave][(unsigned)((key[k] - kb) >> shift) & mask], 1u);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < ND / PT; q++) {
    const int d = q * PT + threadIdx.x;
    table[(size_t)blockIdx.x * ND + d] = cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d];
  }
}

// thread = digit (and digit + 256): the tiles [t0, t1) in turn, their counts replaced by the running count before them
template <int ND>
__device__ inline void rss_walk(unsigned* __restrict__ table, int t0, int t1, unsigned (&run)[ND / PT]) {
  // 16 rows' loads in flight: the walk is a chain of memory round trips, not of adds
#pragma unroll 16
  for (int t = t0; t < t1; t++)
#pragma unroll
    for (int q = 0; q < ND / PT; q++) {
      const size_t at = (size_t)t * ND + q * PT + threadIdx.x;
      const unsigned v = table[at];
      table[at] = run[q];
      run[q] += v;
    }
}

template <int ND>
__global__ __launch_bounds__(PT) void k_rss_chunks(unsigned* __restrict__ table, GhRsSegs S, unsigned* __restrict__ part) {
  const int c = (int)blockIdx.x, seg = gh_rs_find(S.coff, S.nseg, c);
  const int t0 = S.toff[seg] + (c - S.coff[seg]) * RC, t1 = t0 + RC < S.toff[seg + 1] ? t0 + RC : S.toff[seg + 1];
  unsigned run[ND / PT] = {};
  rss_walk<ND>(table, t0, t1, run);
#pragma unroll
  for (int q = 0; q < ND / PT; q++) part[(size_t)c * ND + q * PT + threadIdx.x] = run[q];
}

// One workgroup per segment: the chunks' totals -> part[chunk][digit] = items of the segment with a lower digit + items of that digit in the
// segment's chunks before.  walk: the segment is one chunk whose tiles this kernel walks itself (no k_rss_chunks before it).
template <int ND>
__global__ __launch_bounds__(PT) void k_rss_bases(unsigned* __restrict__ table, unsigned* __restrict__ part, GhRsSegs S, int walk) {
  constexpr int DPT = ND / PT;
  __shared__ unsigned sh[4];
  __shared__ unsigned dig[ND];
  const int s = (int)blockIdx.x, c0 = S.coff[s], c1 = S.coff[s + 1];
  if (c0 == c1) return;  // an empty segment
  unsigned run[DPT] = {};
  if (walk) rss_walk<ND>(table, S.toff[s], S.toff[s + 1], run);
  else
    for (int c = c0; c < c1; c++)
#pragma unroll
      for (int q = 0; q < DPT; q++) {
        const size_t at = (size_t)c * ND + q * PT + threadIdx.x;
        const unsigned v = part[at];
        part[at] = run[q];
        run[q] += v;
      }
#pragma unroll
  for (int q = 0; q < DPT; q++) dig[q * PT + threadIdx.x] = run[q];
  __syncthreads();
  unsigned sum[DPT], all = 0;  // DPT consecutive digits per thread for the scan over the digits
#pragma unroll
  for (int q = 0; q < DPT; q++) { sum[q] = dig[threadIdx.x * DPT + q]; all += sum[q]; }
  unsigned tot;
  unsigned ex = block_excl_scan(all, sh, &tot);
#pragma unroll
  for (int q = 0; q < DPT; q++) { dig[threadIdx.x * DPT + q] = ex; ex += sum[q]; }
  __syncthreads();
  if (walk) {
#pragma unroll
    for (int q = 0; q < DPT; q++) part[(size_t)c0 * ND + q * PT + threadIdx.x] = dig[q * PT + threadIdx.x];
  } else {
    for (int c = c0; c < c1; c++)
#pragma unroll
      for (int q = 0; q < DPT; q++) part[(size_t)c * ND + q * PT + threadIdx.x] += dig[q * PT + threadIdx.x];
  }
}

template <typename K, bool HASV, int ND>
__global__ __launch_bounds__(PT) void k_rss_scatter(const K* __restrict__ kin, const unsigned* __restrict__ vin, K* __restrict__ kout, unsigned* __restrict__ vout,
                                                    GhRsSegs S, const unsigned* __restrict__ kbase, int shift, unsigned mask, const unsigned* __restrict__ table,
                                                    const unsigned* __restrict__ part) {
  constexpr int DPT = ND / PT;
  __shared__ RsTile<K, HASV, ND> T;
  __shared__ unsigned s_delta[ND];  // global position of the digit's run of this tile - its first position in the tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const GhRsTile t = gh_rs_tile(S, (int)blockIdx.x);
  const K kb = kbase ? (K)kbase[t.seg] : (K)0;
  K key[PI];
  unsigned val[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const int j = (wave * PI + k) * 64 + lane;
    key[k] = j < t.here ? kin[(size_t)t.first + j] : (K)0;
    val[k] = (HASV && j < t.here) ? vin[(size_t)t.first + j] : 0u;
  }
  const int chunk = S.coff[t.seg] + ((int)blockIdx.x - S.toff[t.seg]) / RC;
  unsigned run_at[DPT];
#pragma unroll
  for (int q = 0; q < DPT; q++) {
    const int d = q * PT + threadIdx.x;
    run_at[q] = (unsigned)S.off[t.seg] + table[(size_t)blockIdx.x * ND + d] + part[(size_t)chunk * ND + d];
  }
  rs_tile_sort<K, HASV, ND>(T, key, val, t.here, shift, mask, kb);
#pragma unroll
  for (int q = 0; q < DPT; q++) {
    const int d = q * PT + threadIdx.x;
    s_delta[d] = run_at[q] - (unsigned)T.first[d];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PI; j++) {
    const int p = j * PT + threadIdx.x;
    if (p < t.here) {
      const K kk = T.lk[p];
      const unsigned pos = s_delta[(unsigned)((kk - kb) >> shift) & mask] + (unsigned)p;
      kout[pos] = kk;
      if (HASV) vout[pos] = T.lv[p];
    }
  }
}

// no segment beyond one tile: every place in ONE launch, a workgroup per segment (k_rs_small per segment)
template <typename K, bool HASV, int ND>
__global__ __launch_bounds__(PT) void k_rss_small(const K* __restrict__ kin, const unsigned* __restrict__ vin, K* __restrict__ kout, unsigned* __restrict__ vout,
                                                  GhRsSegs S, const unsigned* __restrict__ kbase, int bit_begin, GhRsPlan P) {
  __shared__ RsTile<K, HASV, ND> T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = (int)blockIdx.x, n = S.off[s + 1] - S.off[s];
  if (n <= 0) return;
  const size_t at = (size_t)S.off[s];
  const K kb = kbase ? (K)kbase[s] : (K)0;
  K key[PI];
  unsigned val[PI];
#pragma unroll
  for (int k = 0; k < PI; k++) {
    const int i = (wave * PI + k) * 64 + lane;
    key[k] = i < n ? kin[at + i] : (K)0;
    val[k] = (HASV && i < n) ? vin[at + i] : 0u;
  }
  int shift = bit_begin;
  for (int p = 0; p < P.places; p++) {
    rs_tile_sort<K, HASV, ND>(T, key, val, n, shift, (1u << P.width[p]) - 1u, kb);
    shift += P.width[p];
    if (p + 1 < P.places) {
#pragma unroll
      for (int k = 0; k < PI; k++) {
        const int i = (wave * PI + k) * 64 + lane;
        if (i < n) {
          key[k] = T.lk[i];
          if (HASV) val[k] = T.lv[i];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PI; j++) {
    const int p = j * PT + threadIdx.x;
    if (p < n) {
      kout[at + p] = T.lk[p];
      if (HASV) vout[at + p] = T.lv[p];
    }
  }
}

// one place.  first: the counts of this place are in the table already (GhRsFirst: the kernel that made the keys took them)
template <typename K, bool HASV, int ND>
void rss_place(hipStream_t s, const K* src_k, const unsigned* src_v, K* dst_k, unsigned* dst_v, const GhRsSegs& S, bool one_chunk, const unsigned* kbase, int shift,
               unsigned mask, unsigned* table, unsigned* part, bool first) {
  const int nt = S.toff[S.nseg], nchunk = S.coff[S.nseg];
  if (!first) hipLaunchKernelGGL((k_rss_hist<K, ND>), dim3(nt), dim3(PT), 0, s, src_k, S, kbase, shift, mask, table);
  if (!one_chunk) hipLaunchKernelGGL((k_rss_chunks<ND>), dim3(nchunk), dim3(PT), 0, s, table, S, part);
  hipLaunchKernelGGL((k_rss_bases<ND>), dim3(S.nseg), dim3(PT), 0, s, table, part, S, one_chunk ? 1 : 0);
  hipLaunchKernelGGL((k_rss_scatter<K, HASV, ND>), dim3(nt), dim3(PT), 0, s, src_k, src_v, dst_k, dst_v, S, kbase, shift, mask, (const unsigned*)table,
                     (const unsigned*)part);
}

bool rs_wide(const GhRsPlan& P) {  // a 9-bit place among them
  bool wide = false;
  for (int p = 0; p < P.places; p++) wide = wide || P.width[p] > 8;
  return wide;
}
// the table of a tiled sort: table[tile][nd], then part[chunk][nd] (nd: the widest place's)
int rs_table(ghicp_ctx* ctx, const GhRsSort& R, unsigned** table, unsigned** part) {
  const size_t nd = rs_wide(R.P) ? 512 : 256, nt = (size_t)R.S.toff[R.S.nseg], nchunk = (size_t)R.S.coff[R.S.nseg];
  GH_TRY(ctx->reserve(B_PRIM_TMP, nt * nd + nchunk * nd + 4, table));
  *part = *table + nt * nd;
  return GHICP_OK;
}

// test hook (ghicp_ctx_set_sort_hist_check): the counts a key-making kernel left against k_rss_hist's over the same keys; synchronises
template <typename K>
int rs_check_first(ghicp_ctx* ctx, const GhRsSort& R, const K* kin, const unsigned* kbase, int bit_begin, unsigned* table) {
  const size_t words = (size_t)R.S.toff[R.S.nseg] * (size_t)R.first.nd;
  std::vector<unsigned> left(words), own(words);
  GH_HIP(hipMemcpyAsync(left.data(), table, words * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  if (R.first.nd == 512) hipLaunchKernelGGL((k_rss_hist<K, 512>), dim3(R.S.toff[R.S.nseg]), dim3(PT), 0, ctx->stream, kin, R.S, kbase, bit_begin, R.first.mask, table);
  else hipLaunchKernelGGL((k_rss_hist<K, 256>), dim3(R.S.toff[R.S.nseg]), dim3(PT), 0, ctx->stream, kin, R.S, kbase, bit_begin, R.first.mask, table);
  GH_HIP(hipMemcpyAsync(own.data(), table, words * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  ctx->sort_hist_checked++;
  if (left != own) {
    ctx->sort_hist_mismatched++;
    return ctx->fail(GHICP_ERR_INTERNAL, "segmented sort: the first place's counts left by the key kernel differ from the keys' own");
  }
  return GHICP_OK;
}

template <typename K>
int radix_sort_seg_impl(ghicp_ctx* ctx, const K* kin, K* kout, const unsigned* vin, unsigned* vout, const GhRsSort& R, const unsigned* kbase, int bit_begin) {
  const GhRsSegs& S = R.S;
  const GhRsPlan& P = R.P;
  const int nseg = S.nseg;
  const long long n = S.off[nseg];
  if (n <= 0) return GHICP_OK;
  hipStream_t s = ctx->stream;
  const bool hasv = vin != nullptr;
  if (P.places == 0) {
    GH_HIP(hipMemcpyAsync(kout, kin, (size_t)n * sizeof(K), hipMemcpyDeviceToDevice, s));
    if (hasv) GH_HIP(hipMemcpyAsync(vout, vin, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    return GHICP_OK;
  }
  const bool wide = rs_wide(P);
  const unsigned* nov = nullptr;
  unsigned* novo = nullptr;
  if (R.longest <= TILE) {
    if (hasv && wide) hipLaunchKernelGGL((k_rss_small<K, true, 512>), dim3(nseg), dim3(PT), 0, s, kin, vin, kout, vout, S, kbase, bit_begin, P);
    else if (hasv) hipLaunchKernelGGL((k_rss_small<K, true, 256>), dim3(nseg), dim3(PT), 0, s, kin, vin, kout, vout, S, kbase, bit_begin, P);
    else if (wide) hipLaunchKernelGGL((k_rss_small<K, false, 512>), dim3(nseg), dim3(PT), 0, s, kin, nov, kout, novo, S, kbase, bit_begin, P);
    else hipLaunchKernelGGL((k_rss_small<K, false, 256>), dim3(nseg), dim3(PT), 0, s, kin, nov, kout, novo, S, kbase, bit_begin, P);
    GH_HIP(hipGetLastError());
    return GHICP_OK;
  }
  unsigned *table, *part;
  GH_TRY(rs_table(ctx, R, &table, &part));
  const bool have_first = R.have_first && R.first.table == table;  // (a table that moved since gh_rs_seg_begin: the counts are taken again)
  if (have_first && ctx->sort_hist_check) GH_TRY(rs_check_first<K>(ctx, R, kin, kbase, bit_begin, table));
  K* spare_k = nullptr;
  unsigned* spare_v = nullptr;
  if (P.places > 1) {  // the input is left alone, as in radix_sort_impl
    char* sp;
    const size_t kb = (((size_t)n * sizeof(K) + 255) / 256) * 256;
    GH_TRY(ctx->reserve(B_GRID_TMP, kb + (hasv ? (size_t)n * sizeof(unsigned) : 0) + 16, &sp));
    spare_k = reinterpret_cast<K*>(sp);
    spare_v = reinterpret_cast<unsigned*>(sp + kb);
  }
  const bool one_chunk = R.longest <= (long long)RC * TILE;
  const K* src_k = kin;
  const unsigned* src_v = vin;
  int shift = bit_begin;
  for (int p = 0; p < P.places; p++) {
    const bool to_out = ((P.places - 1 - p) & 1) == 0;
    K* dst_k = to_out ? kout : spare_k;
    unsigned* dst_v = to_out ? vout : spare_v;
    const unsigned mask = (1u << P.width[p]) - 1u;
    const bool w9 = P.width[p] > 8, first = p == 0 && have_first;
    if (hasv && w9) rss_place<K, true, 512>(s, src_k, src_v, dst_k, dst_v, S, one_chunk, kbase, shift, mask, table, part, first);
    else if (hasv) rss_place<K, true, 256>(s, src_k, src_v, dst_k, dst_v, S, one_chunk, kbase, shift, mask, table, part, first);
    else if (w9) rss_place<K, false, 512>(s, src_k, nov, dst_k, novo, S, one_chunk, kbase, shift, mask, table, part, first);
    else rss_place<K, false, 256>(s, src_k, nov, dst_k, novo, S, one_chunk, kbase, shift, mask, table, part, first);
    shift += P.width[p];
    src_k = dst_k;
    src_v = dst_v;
  }
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

template <int MODE>
int select_impl(ghicp_ctx* ctx, const void* in, long long n, unsigned* out, int* d_count, const unsigned* vals = nullptr) {
  hipStream_t s = ctx->stream;
  if (n <= 0) {
    if (d_count) GH_HIP(hipMemsetAsync(d_count, 0, sizeof(int), s));
    return GHICP_OK;
  }
  const int nt = tiles_of(n);
  unsigned* totals;
  GH_TRY(ctx->reserve(B_PRIM_TMP, (size_t)nt + 2, &totals));
  hipLaunchKernelGGL((k_tile_totals<MODE>), dim3(nt), dim3(PT), 0, s, in, n, totals);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(PT), 0, s, totals, nt, d_count);
  hipLaunchKernelGGL((k_select_apply<MODE>), dim3(nt), dim3(PT), 0, s, in, n, (const unsigned*)totals, out, vals);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

}  // namespace

int gh_scan_inclusive_u32(ghicp_ctx* ctx, unsigned* data, long long n) {
  if (n <= 0) return GHICP_OK;
  hipStream_t s = ctx->stream;
  const int nt = tiles_of(n);
  unsigned* totals;
  GH_TRY(ctx->reserve(B_PRIM_TMP, (size_t)nt + 2, &totals));
  hipLaunchKernelGGL((k_tile_totals<0>), dim3(nt), dim3(PT), 0, s, (const void*)data, n, totals);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(PT), 0, s, totals, nt, (int*)nullptr);
  hipLaunchKernelGGL(k_scan_apply, dim3(nt), dim3(PT), 0, s, data, n, (const unsigned*)totals);
  GH_HIP(hipGetLastError());
  return GHICP_OK;
}

int gh_select_flagged_iota(ghicp_ctx* ctx, const unsigned char* flags, long long n, int* out_idx, int* d_count) {
  return select_impl<1>(ctx, flags, n, reinterpret_cast<unsigned*>(out_idx), d_count);
}

int gh_select_flagged_u32(ghicp_ctx* ctx, const unsigned* vals, const unsigned char* flags, long long n, unsigned* out, int* d_count) {
  return select_impl<1>(ctx, flags, n, out, d_count, vals);
}

int gh_unique_sorted_u32(ghicp_ctx* ctx, const unsigned* keys, long long n, unsigned* out, int* d_count) {
  return select_impl<2>(ctx, keys, n, out, d_count);
}

int gh_radix_sort_u32(ghicp_ctx* ctx, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in, unsigned* vals_out, long long n, int bit_begin,
                      int bit_end) {
  return radix_sort_impl<unsigned>(ctx, keys_in, keys_out, vals_in, vals_out, n, bit_begin, bit_end);
}

int gh_radix_sort_u64(ghicp_ctx* ctx, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* vals_in, unsigned* vals_out, long long n,
                      int bit_begin, int bit_end) {
  return radix_sort_impl<unsigned long long>(ctx, keys_in, keys_out, vals_in, vals_out, n, bit_begin, bit_end);
}

int gh_rs_seg_begin(ghicp_ctx* ctx, int nseg, const int* off, int bits, int max_width, GhRsSort* R) {
  if (nseg <= 0 || nseg > GH_RS_MAX_SEGS || off[0] != 0) return ctx->fail(GHICP_ERR_ARG, "segmented sort: 1 .. %d segments from offset 0", GH_RS_MAX_SEGS);
  R->longest = gh_rs_segs_make(&R->S, nseg, off);
  R->P = gh_rs_plan(bits, max_width ? max_width : ctx->sort_digit_bits);
  R->first.table = nullptr;
  R->first.nd = R->P.places && R->P.width[0] > 8 ? 512 : 256;
  R->first.mask = R->P.places ? (1u << R->P.width[0]) - 1u : 0u;
  R->have_first = false;
  if (R->P.places > 0 && R->longest > TILE) {
    unsigned* part;
    GH_TRY(rs_table(ctx, *R, &R->first.table, &part));
  }
  return GHICP_OK;
}

int gh_radix_sort_seg_u32(ghicp_ctx* ctx, const unsigned* keys_in, unsigned* keys_out, const unsigned* vals_in, unsigned* vals_out, const GhRsSort& R,
                          const unsigned* seg_base, int bit_begin) {
  return radix_sort_seg_impl<unsigned>(ctx, keys_in, keys_out, vals_in, vals_out, R, seg_base, bit_begin);
}

int gh_radix_sort_seg_u64(ghicp_ctx* ctx, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* vals_in, unsigned* vals_out,
                          const GhRsSort& R, int bit_begin) {
  return radix_sort_seg_impl<unsigned long long>(ctx, keys_in, keys_out, vals_in, vals_out, R, nullptr, bit_begin);
}

namespace {
// [a, a + na) and [b, b + nb) share a byte (null ranges share nothing)
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return a != nullptr && b != nullptr && na != 0 && nb != 0 && pa < pb + nb && pb < pa + na;
}
// the grand total a select / unique left in device memory -> *count [host]; synchronises the stream
int fetch_count(ghicp_ctx* ctx, const int* d_count, int64_t* count) {
  int* hc = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->pinned) + 320);  // pinned: see gh_bbox_dev
  GH_HIP(hipMemcpyAsync(hc, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  GH_HIP(hipStreamSynchronize(ctx->stream));
  *count = (int64_t)(unsigned)*hc;
  return GHICP_OK;
}
}  // namespace

extern "C" int ghicp_scan_inclusive_u32(ghicp_ctx* ctx, uint32_t* data, int64_t n) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && n < (1ll << 31) - 2 && (n == 0 || data != nullptr));
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  unsigned* d;
  GH_TRY(sg.out(data, (size_t)n, &d));  // device-pointer mode: d == data, the caller's pointer reaches the kernels as it is
  if (ctx->host_ptrs) GH_HIP(hipMemcpyAsync(d, data, (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
  GH_TRY(gh_scan_inclusive_u32(ctx, d, n));
  return sg.finish();
}

extern "C" int ghicp_select_flagged(ghicp_ctx* ctx, const uint8_t* flags, const uint32_t* vals, int64_t n, uint32_t* out, int64_t* count) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && n < (1ll << 31) - 2 && count != nullptr && (n == 0 || (flags != nullptr && out != nullptr)));
  GH_ARG(!ranges_overlap(out, (size_t)n * 4, flags, (size_t)n) && !ranges_overlap(out, (size_t)n * 4, vals, (size_t)n * 4));
  *count = 0;
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  const unsigned char* f;
  const unsigned* v = nullptr;
  unsigned* o;
  int* dcount;
  GH_TRY(sg.in(flags, (size_t)n, &f));
  if (vals) GH_TRY(sg.in(vals, (size_t)n, &v));
  GH_TRY(sg.out(out, (size_t)n, &o));
  GH_TRY(ctx->reserve(B_FE_SCAN, 16, &dcount));
  if (v) GH_TRY(gh_select_flagged_u32(ctx, v, f, n, o, dcount));
  else GH_TRY(gh_select_flagged_iota(ctx, f, n, reinterpret_cast<int*>(o), dcount));
  GH_TRY(fetch_count(ctx, dcount, count));
  if (!sg.outs.empty()) sg.outs.back().bytes = (size_t)*count * sizeof(unsigned);  // host-pointer mode: only out[0 .. count) is the caller's to lose
  return sg.finish();
}

extern "C" int ghicp_unique_sorted_u32(ghicp_ctx* ctx, const uint32_t* keys, int64_t n, uint32_t* out, int64_t* count) {
  GH_ENTER(ctx);
  GH_ARG(n >= 0 && n < (1ll << 31) - 2 && count != nullptr && (n == 0 || (keys != nullptr && out != nullptr)));
  GH_ARG(!ranges_overlap(out, (size_t)n * 4, keys, (size_t)n * 4));
  *count = 0;
  if (n == 0) return GHICP_OK;
  Stager sg(ctx);
  const unsigned* k;
  unsigned* o;
  int* dcount;
  GH_TRY(sg.in(keys, (size_t)n, &k));
  GH_TRY(sg.out(out, (size_t)n, &o));
  GH_TRY(ctx->reserve(B_FE_SCAN, 16, &dcount));
  GH_TRY(gh_unique_sorted_u32(ctx, k, n, o, dcount));
  GH_TRY(fetch_count(ctx, dcount, count));
  if (!sg.outs.empty()) sg.outs.back().bytes = (size_t)*count * sizeof(unsigned);
  return sg.finish();
}

extern "C" int ghicp_sort_pairs(ghicp_ctx* ctx, int key_bytes, const void* keys_in, void* keys_out, const uint32_t* vals_in, uint32_t* vals_out, int64_t n,
                                int bit_begin, int bit_end) {
  GH_ENTER(ctx);
  GH_ARG((key_bytes == 4 || key_bytes == 8) && n >= 0 && n < (1ll << 31) - 2 && bit_begin >= 0 && bit_begin <= bit_end && bit_end <= 8 * key_bytes);
  GH_ARG((vals_in == nullptr) == (vals_out == nullptr) && (n == 0 || (keys_in != nullptr && keys_out != nullptr && keys_in != keys_out)));
  if (n == 0) return GHICP_OK;
  {  // a pass scatters into an output while other workgroups still read the inputs: no output may share a byte with an input or with the other output
    const size_t kbytes = (size_t)n * (size_t)key_bytes, vbytes = (size_t)n * sizeof(uint32_t);
    GH_ARG(!ranges_overlap(keys_out, kbytes, keys_in, kbytes) && !ranges_overlap(keys_out, kbytes, vals_in, vbytes) && !ranges_overlap(keys_out, kbytes, vals_out, vbytes));
    GH_ARG(!ranges_overlap(vals_out, vbytes, vals_in, vbytes) && !ranges_overlap(vals_out, vbytes, keys_in, kbytes));
  }
  Stager sg(ctx);
  const unsigned* vi = nullptr;
  unsigned* vo = nullptr;
  if (vals_in) {
    GH_TRY(sg.in(vals_in, (size_t)n, &vi));
    GH_TRY(sg.out(vals_out, (size_t)n, &vo));
  }
  if (key_bytes == 4) {
    const unsigned* ki;
    unsigned* ko;
    GH_TRY(sg.in(static_cast<const unsigned*>(keys_in), (size_t)n, &ki));
    GH_TRY(sg.out(static_cast<unsigned*>(keys_out), (size_t)n, &ko));
    GH_TRY(gh_radix_sort_u32(ctx, ki, ko, vi, vo, n, bit_begin, bit_end));
  } else {
    const unsigned long long* ki;
    unsigned long long* ko;
    GH_TRY(sg.in(static_cast<const unsigned long long*>(keys_in), (size_t)n, &ki));
    GH_TRY(sg.out(static_cast<unsigned long long*>(keys_out), (size_t)n, &ko));
    GH_TRY(gh_radix_sort_u64(ctx, ki, ko, vi, vo, n, bit_begin, bit_end));
  }
  return sg.finish();
}

extern "C" int ghicp_sort_segments(ghicp_ctx* ctx, int key_bytes, const void* keys_in, void* keys_out, const uint32_t* vals_in, uint32_t* vals_out, int32_t n_segs,
                                   const int64_t* seg_off, const uint32_t* seg_base, int bit_begin, int bits, int max_digit_bits) {
  GH_ENTER(ctx);
  GH_ARG((key_bytes == 4 || key_bytes == 8) && n_segs >= 1 && n_segs <= GH_RS_MAX_SEGS && seg_off != nullptr && seg_off[0] == 0);
  GH_ARG(bit_begin >= 0 && bits >= 0 && bit_begin + bits <= 8 * key_bytes && (max_digit_bits == 0 || max_digit_bits == 8 || max_digit_bits == 9));
  GH_ARG(seg_base == nullptr || key_bytes == 4);
  int off[GH_RS_MAX_SEGS + 1];
  for (int s = 0; s <= n_segs; s++) {
    GH_ARG(seg_off[s] < (1ll << 31) - 2 && (s == 0 || seg_off[s] >= seg_off[s - 1]));
    off[s] = (int)seg_off[s];
  }
  const int64_t n = seg_off[n_segs];
  GH_ARG((vals_in == nullptr) == (vals_out == nullptr) && (n == 0 || (keys_in != nullptr && keys_out != nullptr && keys_in != keys_out)));
  if (n == 0) return GHICP_OK;
  {
    const size_t kbytes = (size_t)n * (size_t)key_bytes, vbytes = (size_t)n * sizeof(uint32_t);
    GH_ARG(!ranges_overlap(keys_out, kbytes, keys_in, kbytes) && !ranges_overlap(keys_out, kbytes, vals_in, vbytes) && !ranges_overlap(keys_out, kbytes, vals_out, vbytes));
    GH_ARG(!ranges_overlap(vals_out, vbytes, vals_in, vbytes) && !ranges_overlap(vals_out, vbytes, keys_in, kbytes));
  }
  Stager sg(ctx);
  const unsigned *vi = nullptr, *sb = nullptr;
  unsigned* vo = nullptr;
  if (vals_in) {
    GH_TRY(sg.in(vals_in, (size_t)n, &vi));
    GH_TRY(sg.out(vals_out, (size_t)n, &vo));
  }
  if (seg_base) GH_TRY(sg.in(seg_base, (size_t)n_segs, &sb));
  const unsigned *ki4 = nullptr;
  const unsigned long long* ki8 = nullptr;
  unsigned* ko4 = nullptr;
  unsigned long long* ko8 = nullptr;
  if (key_bytes == 4) {
    GH_TRY(sg.in(static_cast<const unsigned*>(keys_in), (size_t)n, &ki4));
    GH_TRY(sg.out(static_cast<unsigned*>(keys_out), (size_t)n, &ko4));
  } else {
    GH_TRY(sg.in(static_cast<const unsigned long long*>(keys_in), (size_t)n, &ki8));
    GH_TRY(sg.out(static_cast<unsigned long long*>(keys_out), (size_t)n, &ko8));
  }
  GhRsSort R;
  GH_TRY(gh_rs_seg_begin(ctx, n_segs, off, bits, max_digit_bits, &R));
  const int rc = key_bytes == 4 ? gh_radix_sort_seg_u32(ctx, ki4, ko4, vi, vo, R, sb, bit_begin) : gh_radix_sort_seg_u64(ctx, ki8, ko8, vi, vo, R, bit_begin);
  GH_TRY(rc);
  return sg.finish();
}

// test hook: with it on, every segmented sort that is handed the first place's counts by a key-making kernel takes them again from the keys and
// compares (a host round trip per sort); the two counters say how many sorts were checked and how many differed
extern "C" int ghicp_ctx_set_sort_hist_check(ghicp_ctx* ctx, int on) {
  GH_ENTER(ctx);
  ctx->sort_hist_check = on != 0;
  return GHICP_OK;
}
extern "C" int ghicp_ctx_sort_hist_checks(ghicp_ctx* ctx, int64_t* checked, int64_t* mismatched) {
  GH_ENTER(ctx);
  GH_ARG(checked != nullptr && mismatched != nullptr);
  *checked = ctx->sort_hist_checked;
  *mismatched = ctx->sort_hist_mismatched;
  return GHICP_OK;
}
