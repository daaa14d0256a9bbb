// Internal: what the single-pair fine registration (icp.hip) and its batched forms over cached clouds (refine.hip, refine_gicp.hip) share -- the
// search grids, the per-pair loop state, and the bodies of the per-iteration kernels.  A body takes the block index within ITS pair
// (and, where a kernel strides over the points, the number of blocks of that pair), so that a batched launch gives every pair the
// block shape, the partial records and the reduction order of the single-pair launch: same sums, bit for bit.
#pragma once
#include "grid.h"
#include "devmath.h"

#include <cmath>
#include <cstdlib>

namespace icpdev {

constexpr float kInf = 3.0e38f;
constexpr int RCAP = 2;     // rings searched per query on the fine grid before it is handed to the coarse grid
constexpr int NBLK = 512;   // partial-sum blocks of the accumulation kernels
constexpr int NPART = 32;   // doubles per partial record

struct NnGrid {
  GridDesc d;
  const float4* pts;
  const unsigned* start;
  float cell;
};

struct NnIndex {
  NnGrid fine, coarse;
};

struct IcpState {
  float T[16];    // transformation_ of this iteration
  float fin[16];  // final_transformation_
  double prev_mse, mse, eps_t, eps_e;
  float msf[3], mtf[3];
  int iterations, max_iter, converged, reason;
  unsigned count, nv;  // valid correspondences / kept after trimming
  int trimmed, metric;
  float ratio;
  unsigned pend;
  // radix select of the trimming threshold K* = (d2star, istar): correspondences with a smaller (d2 bits, index) are kept
  unsigned sel_prefix[6], sel_rank[6];
  unsigned d2star, istar;
  int sel_done;
  // batched loop (refine.hip) only: a pair the overlap gate refused (or an empty one) never runs; the sum behind getFitnessScore()
  int refused;
  double fit_sum;
};

// A pair of a batch that has left its loop -- converged, stopped without correspondences, or refused -- is FROZEN: the single-pair loop
// stops launching for it, so no block of a batched launch may touch its points, its state or its partial records again.  One test for
// both loop states (IcpState; GicpState below: converged, out of iterations, fewer than 4 correspondences, refused).
template <typename State>
__device__ inline bool frozen(const State* st) { return st->refused || st->converged || st->reason == GHICP_ICP_NO_CORRESPONDENCES; }

// ------------------------------------------------------------------------------------------------ 1-NN search
// Rounding margin of axis a: how far beyond the face mn + k * cell a point assigned to cell k may lie.  The cell of a point
// is floor((v - mn) * inv), three float roundings plus that of cell = 1 / inv: an error of up to 2.4e-7 * k cells at cell
// k, so the margin grows with the cells of the axis (a 0.02 m cell along a line of 400 m is 20 000 cells) on top of a
// flat 2e-3 cell.  The rounding of mn + k * cell itself is monotone and cannot put a float on the wrong side of a face.
__device__ inline float axis_margin(const NnGrid& G, int a) { return (2e-3f + 4e-7f * (float)G.d.dim[a]) * G.cell; }

// Lower bound on the distance from p to any point in a cell outside the block [c - r, c + r]^3 (sides clipped by the
// grid need no bound: nothing lies beyond them).  The margin is SUBTRACTED: a point of a cell outside the block may lie
// that far inside the block's faces.
__device__ inline float block_reach(const NnGrid& G, float px, float py, float pz, int cx, int cy, int cz, int r) {
  float m = kInf;
  const float p[3] = {px, py, pz};
  const int c[3] = {cx, cy, cz};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float mg = axis_margin(G, a);
    if (c[a] - r > 0) m = fminf(m, p[a] - (G.d.mn[a] + (float)(c[a] - r) * G.cell) - mg);
    if (c[a] + r < G.d.dim[a] - 1) m = fminf(m, (G.d.mn[a] + (float)(c[a] + r + 1) * G.cell) - p[a] - mg);
  }
  return m;
}

// Lower bound on the squared distance from coordinate p to any point the grid assigns to the cells [lo, hi] of one axis.
// Callers skip a run when this exceeds the best distance so far, so it must never over-estimate: the interval is WIDENED
// by the margin on both sides (a point on a cell face, or a hair beyond it, may be assigned to either neighbour; when
// every target sits on a face -- a line or a thin bar along an axis has y = z = mn -- that decides which runs are read).
__device__ inline float axis_gap2(const NnGrid& G, int a, float p, int lo, int hi) {
  const float m = axis_margin(G, a);
  const float l = G.d.mn[a] + (float)lo * G.cell - m, h = G.d.mn[a] + (float)(hi + 1) * G.cell + m;
  const float d = fmaxf(fmaxf(l - p, p - h), 0.f);
  return d * d;
}

// The cells of block r that are not in block rlo (rlo = -1: the whole block), as z-contiguous runs of the point array.
// bound(x) is called before every x slab and returns the squared distance beyond which a run cannot matter; runs whose
// box lies farther than that from P are skipped (a point at exactly the bound still ties, hence the strict test).
template <typename B, typename F>
__device__ inline void for_shell_runs(const NnGrid& G, float px, float py, float pz, int cx, int cy, int cz, int rlo, int r, B&& bound, F&& f) {
  const GridDesc& g = G.d;
  const unsigned* __restrict__ start = G.start;
  const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
  const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dim[1] - 1);
  const int zl = max(cz - r, 0), zh = min(cz + r, g.dim[2] - 1);
  for (int x = x0; x <= x1; x++) {
    const float lim = bound(x);
    const float gx = axis_gap2(G, 0, px, x, x);
    if (gx > lim) continue;
    for (int y = y0; y <= y1; y++) {
      const float gxy = gx + axis_gap2(G, 1, py, y, y);
      if (gxy > lim) continue;
      const unsigned base = ((unsigned)x * g.dim[1] + y) * g.dim[2];
      if (max(abs(x - cx), abs(y - cy)) > rlo) {
        if (gxy + axis_gap2(G, 2, pz, zl, zh) > lim) continue;
        const unsigned b = start[base + zl], e = start[base + zh + 1];
        if (e > b) f(b, e);
      } else {
        const int a1 = min(cz - rlo - 1, g.dim[2] - 1);
        if (zl <= a1 && !(gxy + axis_gap2(G, 2, pz, zl, a1) > lim)) {
          const unsigned b = start[base + zl], e = start[base + a1 + 1];
          if (e > b) f(b, e);
        }
        const int b0 = max(cz + rlo + 1, 0);
        if (b0 <= zh && !(gxy + axis_gap2(G, 2, pz, b0, zh) > lim)) {
          const unsigned b = start[base + b0], e = start[base + zh + 1];
          if (e > b) f(b, e);
        }
      }
    }
  }
}

__device__ inline void nn_fine_body(const NnGrid& G, const float4* __restrict__ q, int nq, int i, int* __restrict__ nn, float* __restrict__ nd,
                                    unsigned* __restrict__ pend_list, unsigned* __restrict__ pend_count) {
  if (i >= nq) return;
  const float4 P = q[i];
  const int cx = gh_cell_coord(P.x, G.d.mn[0], G.d.inv, G.d.dim[0]);
  const int cy = gh_cell_coord(P.y, G.d.mn[1], G.d.inv, G.d.dim[1]);
  const int cz = gh_cell_coord(P.z, G.d.mn[2], G.d.inv, G.d.dim[2]);
  float bd = kInf;
  int bi = -1;
  bool done = false;
  int rlo = -1;
  for (int r = 1; r <= RCAP; r++) {
    for_shell_runs(G, P.x, P.y, P.z, cx, cy, cz, rlo, r, [&](int) { return bd; }, [&](unsigned b, unsigned e) {
      for (unsigned t = b; t < e; t++) {
        const float4 Q = G.pts[t];
        const int qi = (int)__float_as_uint(Q.w);
        const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        if (d2 < bd || (d2 == bd && qi < bi)) { bd = d2; bi = qi; }
      }
    });
    rlo = r;
    const float reach = block_reach(G, P.x, P.y, P.z, cx, cy, cz, r);
    if (reach >= kInf || (reach > 0.f && bd < reach * reach)) { done = true; break; }
  }
  nn[i] = bi;
  nd[i] = bd;
  if (!done) pend_list[atomicAdd(pend_count, 1u)] = (unsigned)i;
}

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

// One wave per unresolved query, seeded with the fine-grid candidate; ring expansion without a cap.
__device__ inline void nn_coarse_body(const NnGrid& G, const float4* __restrict__ q, const unsigned* __restrict__ pend_list, unsigned np, unsigned w0,
                                      unsigned nw, int* __restrict__ nn, float* __restrict__ nd) {
  const int lane = threadIdx.x & 63;
  for (unsigned w = w0; w < np; w += nw) {
    const unsigned i = pend_list[w];
    const float4 P = q[i];
    const int cx = gh_cell_coord(P.x, G.d.mn[0], G.d.inv, G.d.dim[0]);
    const int cy = gh_cell_coord(P.y, G.d.mn[1], G.d.inv, G.d.dim[1]);
    const int cz = gh_cell_coord(P.z, G.d.mn[2], G.d.inv, G.d.dim[2]);
    unsigned long long best = ((unsigned long long)__float_as_uint(nd[i]) << 32) | (unsigned)nn[i];
    for (int r = 0;; r++) {
      // Shell r as 2 slots per (x, y) column of the block: a rim column is one z run (slot 0), an interior column its two
      // cap cells.  The lanes look the slots up in parallel (box test against the wave's best, then the cell table), then
      // the wave walks the non-empty runs together: no serial chain of table lookups per column.
      const int side = 2 * r + 1, slots = 2 * side * side;
      for (int s0 = 0; s0 < slots; s0 += 64) {
        best = wave_min_u64(best);
        const float lim = __uint_as_float((unsigned)(best >> 32));
        unsigned rb = 0, re = 0;
        const int sl = s0 + lane;
        if (sl < slots) {
          const int c = sl >> 1, h = sl & 1;
          const int x = cx + c / side - r, y = cy + c % side - r;
          if (x >= 0 && x < G.d.dim[0] && y >= 0 && y < G.d.dim[1]) {
            const bool rim = max(abs(x - cx), abs(y - cy)) == r;
            int zl, zh;
            if (rim) { zl = cz - r; zh = h ? zl - 1 : cz + r; }
            else { zl = zh = h ? cz + r : cz - r; }
            if (r == 0 && h) zh = zl - 1;
            zl = max(zl, 0); zh = min(zh, G.d.dim[2] - 1);
            if (zl <= zh && !(axis_gap2(G, 0, P.x, x, x) + axis_gap2(G, 1, P.y, y, y) + axis_gap2(G, 2, P.z, zl, zh) > lim)) {
              const unsigned base = ((unsigned)x * G.d.dim[1] + y) * G.d.dim[2];
              rb = G.start[base + zl];
              re = G.start[base + zh + 1];
            }
          }
        }
        unsigned long long live = __ballot(re > rb);
        while (live) {
          const int l = __ffsll((long long)live) - 1;
          live &= live - 1;
          const unsigned b = __shfl(rb, l, 64), e = __shfl(re, l, 64);
          for (unsigned t = b + lane; t < e; t += 64) {
            const float4 Q = G.pts[t];
            const float dx = P.x - Q.x, dy = P.y - Q.y, dz = P.z - Q.z;
            float d2 = dx * dx;
            d2 += dy * dy;
            d2 += dz * dz;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(Q.w);
            best = key < best ? key : best;
          }
        }
      }
      best = wave_min_u64(best);
      const float bd = __uint_as_float((unsigned)(best >> 32));
      const float reach = block_reach(G, P.x, P.y, P.z, cx, cy, cz, r);
      if (reach >= kInf || (reach > 0.f && bd < reach * reach)) break;
    }
    if (lane == 0) {
      nn[i] = (int)(unsigned)best;
      nd[i] = __uint_as_float((unsigned)(best >> 32));
    }
  }
}

// adds the number of threads of a 256-thread block with `flag` set to *dst: one atomic per block
__device__ inline void block_count_add(bool flag, unsigned* dst) {
  __shared__ unsigned wsum[4];
  const unsigned long long b = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (t) atomicAdd(dst, t);
  }
}

// calOverlap of one query (common_reg.cpp:294-317): does the target hold a point at d^2 < r2?  G has a cell >= the radius: a query outside
// the padded grid has no neighbour; inside, the 27 cells around it hold every candidate.  Shared by k_overlap (icp.hip) and the batched
// k_ov_pairs (overlap_clouds.hip).
__device__ inline bool overlap_hit(const NnGrid& G, float px, float py, float pz, float r2) {
  bool hit = false;
  const float fx = (px - G.d.mn[0]) * G.d.inv, fy = (py - G.d.mn[1]) * G.d.inv, fz = (pz - G.d.mn[2]) * G.d.inv;
  if (fx >= -1.f && fy >= -1.f && fz >= -1.f && fx <= (float)G.d.dim[0] + 1.f && fy <= (float)G.d.dim[1] + 1.f && fz <= (float)G.d.dim[2] + 1.f) {
    const int cx = gh_cell_coord(px, G.d.mn[0], G.d.inv, G.d.dim[0]);
    const int cy = gh_cell_coord(py, G.d.mn[1], G.d.inv, G.d.dim[1]);
    const int cz = gh_cell_coord(pz, G.d.mn[2], G.d.inv, G.d.dim[2]);
    gh_for_runs(G.d, G.start, cx, cy, cz, [&](unsigned b, unsigned e) {
      for (unsigned t = b; t < e && !hit; t++) {
        const float4 Q = G.pts[t];
        const float dx = px - Q.x, dy = py - Q.y, dz = pz - Q.z;
        float d2 = dx * dx;
        d2 += dy * dy;
        d2 += dz * dz;
        if (d2 < r2) hit = true;
      }
    });
  }
  return hit;
}

// CorrespondenceRejectorTrimmed::getRemainingCorrespondences: floor(overlap_ratio * float(size)).  State: IcpState, or the select record of
// the trimmed generalized ICP (GicpSel below) -- one rule, one select for both loops
template <typename State>
__device__ inline void icp_prep_body(State* st) {
  unsigned nv = st->count;
  if (st->trimmed) {
    const unsigned t = (unsigned)(int)floorf(st->ratio * (float)st->count);
    if (t < nv) nv = t;
  }
  st->nv = nv;
  st->sel_prefix[0] = 0;
  st->sel_rank[0] = nv;
  st->sel_done = nv >= st->count;  // nothing to trim: every valid correspondence is kept
  st->d2star = 0xffffffffu;
  st->istar = 0xffffffffu;
}

// ---- trimmed rejector without a sort.  The kept set is {key < K*} with key = (d2 bits, source index) and K* the key of
// rank nv: an MSD radix select, three digit passes (11 + 11 + 10 bits) over the distance bits, then -- only when ties at
// the threshold distance have to be split -- three over the index bits.  Every pass is one histogram kernel whose blocks
// first derive the prefix chosen so far from the previous pass's histogram.
constexpr int SEL_BINS = 2048;
__device__ inline int sel_bits(int p) { return (p % 3 == 2) ? 10 : 11; }
__device__ inline int sel_shift(int p) { return (p % 3 == 0) ? 21 : ((p % 3 == 1) ? 10 : 0); }

// bin of `hist` (SEL_BINS entries) that holds rank r; *below = entries in lower bins.  Block-cooperative, 256 threads.
__device__ inline unsigned sel_pick(const unsigned* __restrict__ hist, unsigned r, unsigned* below, int* scan_s, unsigned* pick_s) {
  unsigned c[8], sum = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) { c[k] = hist[threadIdx.x * 8 + k]; sum += c[k]; }
  int tot;
  const unsigned ex = (unsigned)gh_block_excl_scan((int)sum, scan_s, &tot);
  if (r >= ex && r < ex + sum) {
    unsigned acc = ex;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (r >= acc && r < acc + c[k]) { pick_s[0] = threadIdx.x * 8 + k; pick_s[1] = acc; }
      acc += c[k];
    }
  }
  __syncthreads();
  *below = pick_s[1];
  return pick_s[0];
}

template <typename State>
__device__ inline void sel_pass_body(int pass, const int* __restrict__ nn, const float* __restrict__ nd, int n, State* __restrict__ st,
                                     unsigned* __restrict__ hist, unsigned blk, unsigned nblk) {
  if (st->sel_done || (pass > 3 && st->istar == 0)) return;
  __shared__ unsigned lh[SEL_BINS];
  __shared__ int scan_s[20];
  __shared__ unsigned pick_s[2];
  unsigned prefix = 0, rank = st->sel_rank[0], d2star = st->d2star;
  if (pass > 0) {
    unsigned below;
    const unsigned bin = sel_pick(hist + (size_t)(pass - 1) * SEL_BINS, st->sel_rank[pass - 1], &below, scan_s, pick_s);
    prefix = (st->sel_prefix[pass - 1] << sel_bits(pass - 1)) | bin;
    rank = st->sel_rank[pass - 1] - below;
    if (pass == 3) {  // the distance is fixed: `rank` of its ties (lowest indices first) are kept
      d2star = prefix;
      prefix = 0;
      if (blk == 0 && threadIdx.x == 0) {
        st->d2star = d2star;
        if (rank == 0) st->istar = 0;
      }
      if (rank == 0) return;  // K* is the first tie: no index digits needed (k_sel_final sees rank 0 too)
    }
    if (blk == 0 && threadIdx.x == 0) { st->sel_prefix[pass] = prefix; st->sel_rank[pass] = rank; }
  }
  for (int k = threadIdx.x; k < SEL_BINS; k += 256) lh[k] = 0;
  __syncthreads();
  const int shift = sel_shift(pass), bits = sel_bits(pass);
  for (int i = blk * 256 + threadIdx.x; i < n; i += nblk * 256) {
    if (nn[i] < 0) continue;
    const unsigned db = __float_as_uint(nd[i]);
    unsigned v;
    bool member;
    if (pass < 3) { v = db; member = pass == 0 || (v >> (shift + bits)) == prefix; }
    else { v = (unsigned)i; member = db == d2star && (pass == 3 || (v >> (shift + bits)) == prefix); }
    if (member) atomicAdd(&lh[(v >> shift) & ((1u << bits) - 1u)], 1u);
  }
  __syncthreads();
  unsigned* out = hist + (size_t)pass * SEL_BINS;
  for (int k = threadIdx.x; k < SEL_BINS; k += 256)
    if (lh[k]) atomicAdd(&out[k], lh[k]);
}

template <typename State>
__device__ inline void sel_final_body(State* __restrict__ st, const unsigned* __restrict__ hist) {
  if (st->sel_done) return;
  __shared__ int scan_s[20];
  __shared__ unsigned pick_s[2];
  if (st->istar == 0) return;  // decided at pass 3
  unsigned below;
  const unsigned bin = sel_pick(hist + (size_t)5 * SEL_BINS, st->sel_rank[5], &below, scan_s, pick_s);
  if (threadIdx.x == 0) st->istar = (st->sel_prefix[5] << 10) | bin;
}

struct CorrView {
  const int* nn;
  const float* nd;
  const float4* cur;
  const float4* tgt;
  int ns;
};

// source point e -> its target j if the correspondence survives the rejectors, else -1: its key (d2 bits, source index) lies below the
// threshold K* of the select (nothing to trim: K* is the largest key).  State: IcpState, or the trimmed generalized ICP's GicpSel
template <typename State>
__device__ inline int corr_at(const CorrView& V, const State* __restrict__ st, unsigned e, int* j) {
  *j = V.nn[e];
  if (*j < 0) return -1;
  const unsigned db = __float_as_uint(V.nd[e]);
  return (db < st->d2star || (db == st->d2star && e < st->istar)) ? (int)e : -1;
}

__device__ inline void store_partials(const double* v, int nv, double* red, double* __restrict__ part, unsigned blk) {
  for (int d = 0; d < nv; d++) {
    const double s = gh_block_sum(v[d], red);
    if (threadIdx.x == 0) part[(size_t)blk * NPART + d] = s;
  }
}

__device__ inline void acc_means_body(const CorrView& V, const IcpState* __restrict__ st, double* __restrict__ part, unsigned blk) {
  __shared__ double red[16];
  const unsigned lim = (unsigned)V.ns;
  double m[7] = {0, 0, 0, 0, 0, 0, 0};
  for (unsigned e = blk * 256u + threadIdx.x; e < lim; e += NBLK * 256u) {
    int j;
    const int i = corr_at(V, st, e, &j);
    if (i < 0) continue;
    const float4 S = V.cur[i], D = V.tgt[j];
    m[0] += (double)S.x; m[1] += (double)S.y; m[2] += (double)S.z;
    m[3] += (double)D.x; m[4] += (double)D.y; m[5] += (double)D.z;
    m[6] += (double)V.nd[i];
  }
  store_partials(m, 7, red, part, blk);
}

// sum of component d over the NBLK block partials by one wave: lane l adds blocks l, l+64, ... then a fixed shuffle tree
__device__ inline double wave_reduce_partials(const double* __restrict__ part, int d) {
  double s = 0;
  for (int b = threadIdx.x; b < NBLK; b += 64) s += part[(size_t)b * NPART + d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

__device__ inline void icp_means_body(IcpState* st, const double* __restrict__ part) {
  double m[7];
  for (int d = 0; d < 7; d++) m[d] = wave_reduce_partials(part, d);
  if (threadIdx.x != 0) return;
  const double c = (double)st->nv;
  for (int d = 0; d < 3; d++) { st->msf[d] = (float)(m[d] / c); st->mtf[d] = (float)(m[3 + d] / c); }
  st->mse = m[6] / c;  // DefaultConvergenceCriteria::calculateMSE over the remaining correspondences
}

__device__ inline void acc_cov_body(const CorrView& V, const IcpState* __restrict__ st, double* __restrict__ part, unsigned blk) {
  __shared__ double red[16];
  const unsigned lim = (unsigned)V.ns;
  const double ms[3] = {(double)st->msf[0], (double)st->msf[1], (double)st->msf[2]};
  const double mt[3] = {(double)st->mtf[0], (double)st->mtf[1], (double)st->mtf[2]};
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned e = blk * 256u + threadIdx.x; e < lim; e += NBLK * 256u) {
    int j;
    const int i = corr_at(V, st, e, &j);
    if (i < 0) continue;
    const float4 S = V.cur[i], D = V.tgt[j];
    const double a[3] = {(double)D.x - mt[0], (double)D.y - mt[1], (double)D.z - mt[2]};
    const double b[3] = {(double)S.x - ms[0], (double)S.y - ms[1], (double)S.z - ms[2]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 3; q++) H[r * 3 + q] += a[r] * b[q];
  }
  store_partials(H, 9, red, part, blk);
}

// TransformationEstimationPointToPlaneLLS: rows [n x s ; n], rhs n.(d - s), float terms summed in f64
__device__ inline void acc_plane_body(const CorrView& V, const float* __restrict__ tnrm, const IcpState* __restrict__ st, double* __restrict__ part,
                                      unsigned blk) {
  __shared__ double red[16];
  const unsigned lim = (unsigned)V.ns;
  double acc[28];
#pragma unroll
  for (int d = 0; d < 28; d++) acc[d] = 0;
  for (unsigned e = blk * 256u + threadIdx.x; e < lim; e += NBLK * 256u) {
    int j;
    const int i = corr_at(V, st, e, &j);
    if (i < 0) continue;
    const float4 S = V.cur[i], D = V.tgt[j];
    const float nx = tnrm[(size_t)j * 3], ny = tnrm[(size_t)j * 3 + 1], nz = tnrm[(size_t)j * 3 + 2];
    const double v[6] = {(double)(nz * S.y - ny * S.z), (double)(nx * S.z - nz * S.x), (double)(ny * S.x - nx * S.y), (double)nx, (double)ny, (double)nz};
    const double dd = (double)(((((nx * D.x + ny * D.y) + nz * D.z) - nx * S.x) - ny * S.y) - nz * S.z);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
      for (int q = r; q < 6; q++) acc[k++] += v[r] * v[q];
    }
#pragma unroll
    for (int r = 0; r < 6; r++) acc[21 + r] += v[r] * dd;
    acc[27] += (double)V.nd[i];
  }
  store_partials(acc, 28, red, part, blk);
}

__device__ inline void mat4_mul(const float* a, const float* b, float* out) {
  float t[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) t[r * 4 + c] = ((a[r * 4] * b[c] + a[r * 4 + 1] * b[4 + c]) + a[r * 4 + 2] * b[8 + c]) + a[r * 4 + 3] * b[12 + c];
  for (int d = 0; d < 16; d++) out[d] = t[d];
}

// closed-form solve + final_transformation_ update + DefaultConvergenceCriteria::hasConverged
__device__ inline void icp_step_body(IcpState* st, const double* __restrict__ part) {
  const unsigned cnt = st->nv;
  double acc[28];
  const int nacc = st->metric == GHICP_ICP_POINT_TO_POINT ? 9 : 28;
  for (int d = 0; d < 28; d++) acc[d] = d < nacc ? wave_reduce_partials(part, d) : 0.0;
  if (threadIdx.x != 0) return;
  if (cnt < 3u) {  // min_number_correspondences_
    st->converged = 0; st->reason = GHICP_ICP_NO_CORRESPONDENCES; st->count = 0;
    return;
  }
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (st->metric == GHICP_ICP_POINT_TO_POINT) {
    double A[9], R[9];
    for (int d = 0; d < 9; d++) A[d] = acc[d] / (double)cnt;
    gh_quant_grid(A, 9);  // N2: umeyama's sigma is a Matrix3f
    gh_kabsch(A, R);
    float Rf[9];
    for (int d = 0; d < 9; d++) Rf[d] = (float)R[d];
    for (int r = 0; r < 3; r++) {
      for (int q = 0; q < 3; q++) T[r * 4 + q] = Rf[r * 3 + q];
      T[r * 4 + 3] = (float)((double)st->mtf[r] - (((double)Rf[r * 3] * (double)st->msf[0] + (double)Rf[r * 3 + 1] * (double)st->msf[1]) +
                                                   (double)Rf[r * 3 + 2] * (double)st->msf[2]));
    }
  } else {
    st->mse = acc[27] / (double)cnt;
    double A[6][6], bb[6], x[6];
    int k = 0;
    for (int r = 0; r < 6; r++)
      for (int q = r; q < 6; q++) { A[r][q] = acc[k]; A[q][r] = acc[k]; k++; }
    for (int r = 0; r < 6; r++) bb[r] = acc[21 + r];
    for (int c = 0; c < 6; c++) {  // elimination with partial pivoting (same sequence as the CPU restatement)
      int piv = c;
      for (int r = c + 1; r < 6; r++) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
      if (piv != c) {
        for (int q = 0; q < 6; q++) { const double t = A[c][q]; A[c][q] = A[piv][q]; A[piv][q] = t; }
        const double t = bb[c]; bb[c] = bb[piv]; bb[piv] = t;
      }
      for (int r = c + 1; r < 6; r++) {
        const double f = A[r][c] / A[c][c];
        for (int q = c; q < 6; q++) A[r][q] -= f * A[c][q];
        bb[r] -= f * bb[c];
      }
    }
    for (int r = 5; r >= 0; r--) {
      double s = bb[r];
      for (int q = r + 1; q < 6; q++) s -= A[r][q] * x[q];
      x[r] = s / A[r][r];
    }
    const double al = x[0], be = x[1], ga = x[2];  // constructTransformationMatrix
    T[0] = (float)(cos(ga) * cos(be));
    T[1] = (float)(-sin(ga) * cos(al) + cos(ga) * sin(be) * sin(al));
    T[2] = (float)(sin(ga) * sin(al) + cos(ga) * sin(be) * cos(al));
    T[4] = (float)(sin(ga) * cos(be));
    T[5] = (float)(cos(ga) * cos(al) + sin(ga) * sin(be) * sin(al));
    T[6] = (float)(-cos(ga) * sin(al) + sin(ga) * sin(be) * cos(al));
    T[8] = (float)(-sin(be));
    T[9] = (float)(cos(be) * sin(al));
    T[10] = (float)(cos(be) * cos(al));
    T[3] = (float)x[3]; T[7] = (float)x[4]; T[11] = (float)x[5];
  }
  for (int d = 0; d < 16; d++) st->T[d] = T[d];
  mat4_mul(T, st->fin, st->fin);
  st->iterations++;
  st->count = 0;
  const double mse = st->mse, prev = st->prev_mse;
  if (st->iterations >= st->max_iter) { st->converged = 1; st->reason = GHICP_ICP_ITERATIONS; return; }
  const double cos_angle = 0.5 * ((double)T[0] + (double)T[5] + (double)T[10] - 1);
  const double tsq = (double)T[3] * T[3] + (double)T[7] * T[7] + (double)T[11] * T[11];
  if (cos_angle >= 1.0 - st->eps_t && tsq <= st->eps_t) { st->converged = 1; st->reason = GHICP_ICP_TRANSFORM; return; }
  if (fabs(mse - prev) < st->eps_e) { st->converged = 1; st->reason = GHICP_ICP_ABS_MSE; return; }
  if (fabs(mse - prev) / prev < 1e-5) { st->converged = 1; st->reason = GHICP_ICP_REL_MSE; return; }
  st->prev_mse = mse;
}

// transformation_ applied to one point: float 4x4 * (x, y, z, 1), the sums in the order of CRegistration::transformcloud
__device__ inline float4 xf_point(const float* M, float x, float y, float z) {
  return make_float4(((M[0] * x + M[1] * y) + M[2] * z) + M[3], ((M[4] * x + M[5] * y) + M[6] * z) + M[7], ((M[8] * x + M[9] * y) + M[10] * z) + M[11], 0.f);
}

__device__ inline void sum_f32_body(const float* __restrict__ v, int n, double* __restrict__ part, unsigned blk) {
  __shared__ double red[16];
  double s = 0;
  for (unsigned e = blk * 256u + threadIdx.x; e < (unsigned)n; e += NBLK * 256u) s += (double)v[e];
  s = gh_block_sum(s, red);
  if (threadIdx.x == 0) part[blk] = s;
}

// ------------------------------------------------------------------------------------------------ generalized ICP
// CRegistration::gicp_reg (common_reg.cpp:216-284) = pcl::GeneralizedIterativeClosestPoint as recalled in ghicp_c.h, with the inner
// solver of DESIGN.md N8.  Per outer iteration: apply, the 1-NN search, mahal, prep, max_inner_iter x (acc, solve), outer, one status
// read.  The inner steps after the stop flag are no-ops.  `blk` is the block within the pair (of NBLK).
struct GicpState {
  float T[16];                   // transformation_
  double x[6];                   // (tx, ty, tz, roll, pitch, yaw) of the inner problem
  double R[9], dR[27];           // R(x) and dR/droll, dR/dpitch, dR/dyaw at x (f64)
  double maxd2, inv_eps_r, inv_eps_t, mse;
  unsigned count;                // correspondences of this iteration
  int iterations, max_iter, converged, reason, inner_done, inner_steps, pad_;
  // batched loop (refine_gicp.hip) only: a pair the overlap gate refused (or an empty one) never runs; the sum behind getFitnessScore()
  int refused;
  float ratio;                   // trimmed loop only: the share of the correspondences within the distance that is kept, fixed for the registration
  double fit_sum;
};

// The trimmed loop (ghicp_gicp_trimmed_from, ghicp_gicp_clouds_trimmed) keeps a select record beside its GicpState: the fields of an
// IcpState that icp_prep_body, sel_pass_body, sel_final_body and corr_at read and write, so the ICP path's rule and radix select serve it
// as they are.  `acc` gathers the survivors of the distance rejection (one integer atomic per block) until the prep step takes it.
struct GicpSel {
  unsigned count, nv;  // within the distance / kept after trimming
  int trimmed;         // 1: the rule of icp_prep_body applies (a ratio of 1 keeps everything)
  float ratio;
  unsigned sel_prefix[6], sel_rank[6];
  unsigned d2star, istar;
  int sel_done;
  unsigned acc;
};

constexpr double kGicpStop = 1e-10;  // N8: the inner loop stops once max |dx| < this

// R(x) = Rz(yaw) Ry(pitch) Rx(roll) and its three partial derivatives, f64
__device__ inline void gicp_rot(const double* x, double* R, double* dR) {
  const double ca = cos(x[3]), sa = sin(x[3]), cb = cos(x[4]), sb = sin(x[4]), cg = cos(x[5]), sg = sin(x[5]);
  const double r[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                       sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                       -sb, cb * sa, cb * ca};
  const double da[9] = {0, cg * sb * ca + sg * sa, -cg * sb * sa + sg * ca,
                        0, sg * sb * ca - cg * sa, -sg * sb * sa - cg * ca,
                        0, cb * ca, -cb * sa};
  const double db[9] = {-cg * sb, cg * cb * sa, cg * cb * ca,
                        -sg * sb, sg * cb * sa, sg * cb * ca,
                        -cb, -sb * sa, -sb * ca};
  const double dg[9] = {-sg * cb, -sg * sb * sa - cg * ca, -sg * sb * ca + cg * sa,
                        cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                        0, 0, 0};
  for (int e = 0; e < 9; e++) { R[e] = r[e]; dR[e] = da[e]; dR[9 + e] = db[e]; dR[18 + e] = dg[e]; }
}

__device__ inline void gicp_state_rot(GicpState* st) {
  double R[9], dR[27];
  gicp_rot(st->x, R, dR);
  for (int e = 0; e < 9; e++) st->R[e] = R[e];
  for (int e = 0; e < 27; e++) st->dR[e] = dR[e];
}

__device__ inline void gicp_apply_body(const float4* __restrict__ src, int n, int i, const GicpState* __restrict__ st, float4* __restrict__ cur) {
  if (i >= n) return;
  const float* M = st->T;
  const float4 P = src[i];
  cur[i] = make_float4(((M[0] * P.x + M[1] * P.y) + M[2] * P.z) + M[3], ((M[4] * P.x + M[5] * P.y) + M[6] * P.z) + M[7],
                       ((M[8] * P.x + M[9] * P.y) + M[10] * P.z) + M[11], 0.f);
}

// M_i = (R C_S,i R^T + C_T,j)^-1 (symmetric: upper triangle of R C R^T + C_T, inverse by cofactors), 6 entries
__device__ inline void gicp_mahal_at(const double* R, const double* cs, const double* ct, double* __restrict__ mahal, unsigned i) {
  const double C[9] = {cs[0], cs[1], cs[2], cs[1], cs[3], cs[4], cs[2], cs[4], cs[5]};
  double P[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) P[r * 3 + c] = (R[r * 3] * C[c] + R[r * 3 + 1] * C[3 + c]) + R[r * 3 + 2] * C[6 + c];
  const int rr[6] = {0, 0, 0, 1, 1, 2}, cc[6] = {0, 1, 2, 1, 2, 2};
  double A[6];
  for (int e = 0; e < 6; e++) {
    const int r = rr[e], c = cc[e];
    A[e] = ((P[r * 3] * R[c * 3] + P[r * 3 + 1] * R[c * 3 + 1]) + P[r * 3 + 2] * R[c * 3 + 2]) + ct[e];
  }
  const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5];
  const double k00 = d * f - e * e, k01 = c * e - b * f, k02 = b * e - c * d, k11 = a * f - c * c, k12 = b * c - a * e, k22 = a * d - b * b;
  const double det = (a * k00 + b * k01) + c * k02;
  double* M = &mahal[(size_t)i * 6];
  M[0] = k00 / det; M[1] = k01 / det; M[2] = k02 / det; M[3] = k11 / det; M[4] = k12 / det; M[5] = k22 / det;
}

// M_i for every correspondence with d^2 < max distance^2; rejected points get nn = -1.  Block partials: [0] accepted count, [1] sum of
// their d^2.
__device__ inline void gicp_mahal_body(int* __restrict__ nn, const float* __restrict__ nd, int ns, const double* __restrict__ covS,
                                       const double* __restrict__ covT, const GicpState* __restrict__ st, double* __restrict__ mahal,
                                       double* __restrict__ part, unsigned blk) {
  __shared__ double red[16];
  double R[9];
  for (int e = 0; e < 9; e++) R[e] = (double)st->T[(e / 3) * 4 + e % 3];
  const double maxd2 = st->maxd2;
  double acc[2] = {0, 0};
  for (unsigned i = blk * 256u + threadIdx.x; i < (unsigned)ns; i += NBLK * 256u) {
    const int j = nn[i];
    if (j < 0) continue;
    if (!((double)nd[i] < maxd2)) { nn[i] = -1; continue; }
    gicp_mahal_at(R, &covS[(size_t)i * 6], &covT[(size_t)j * 6], mahal, i);
    acc[0] += 1.0;
    acc[1] += (double)nd[i];
  }
  store_partials(acc, 2, red, part, blk);
}

// ---- the trimmed loop: the rejector PCL's GICP never consults, applied.  Per outer iteration, after the search: the distance rejection with
// its count (gicp_reject_body), the rule of the ICP path (gicp_trim_prep_body -> icp_prep_body), its radix select over the survivors
// (sel_pass_body / sel_final_body on the GicpSel), then M_i, the count and the MSE over the kept set only (gicp_mahal_trim_body).  The rest of
// the iteration is the untrimmed loop's: gicp_prep_body sees the kept count, fewer than 4 ends the loop.
// Per point: a correspondence with d^2 >= max distance^2 gets nn = -1; the survivors are counted.  Every thread of the block calls this.
__device__ inline void gicp_reject_body(int* __restrict__ nn, const float* __restrict__ nd, int ns, int i, const GicpState* __restrict__ st,
                                        GicpSel* __restrict__ sel) {
  bool keep = false;
  if (i < ns && nn[i] >= 0) {
    keep = (double)nd[i] < st->maxd2;
    if (!keep) nn[i] = -1;
  }
  block_count_add(keep, &sel->acc);
}

// one thread: count = the survivors, nv = min(count, floor(ratio * float(count))), the select's start
__device__ inline void gicp_trim_prep_body(const GicpState* __restrict__ st, GicpSel* __restrict__ sel) {
  sel->count = sel->acc;
  sel->acc = 0;
  sel->trimmed = 1;
  sel->ratio = st->ratio;
  icp_prep_body(sel);
}

// gicp_mahal_body for the kept correspondences (key below K*); the trimmed ones get nn = -1.  Block partials as there, over the kept set.
__device__ inline void gicp_mahal_trim_body(int* __restrict__ nn, const float* __restrict__ nd, int ns, const double* __restrict__ covS,
                                            const double* __restrict__ covT, const GicpState* __restrict__ st, const GicpSel* __restrict__ sel,
                                            double* __restrict__ mahal, double* __restrict__ part, unsigned blk) {
  __shared__ double red[16];
  double R[9];
  for (int e = 0; e < 9; e++) R[e] = (double)st->T[(e / 3) * 4 + e % 3];
  double acc[2] = {0, 0};
  const CorrView V = {nn, nd, nullptr, nullptr, ns};
  for (unsigned i = blk * 256u + threadIdx.x; i < (unsigned)ns; i += NBLK * 256u) {
    int j;
    if (corr_at(V, sel, i, &j) < 0) {
      if (j >= 0) nn[i] = -1;
      continue;
    }
    gicp_mahal_at(R, &covS[(size_t)i * 6], &covT[(size_t)j * 6], mahal, i);
    acc[0] += 1.0;
    acc[1] += (double)nd[i];
  }
  store_partials(acc, 2, red, part, blk);
}

// count and MSE of the correspondences; fewer than 4: PCL throws, the loop ends unconverged.  Else x0 = parameters of transformation_.
__device__ inline void gicp_prep_body(GicpState* st, const double* __restrict__ part) {
  const double cnt = wave_reduce_partials(part, 0), d2 = wave_reduce_partials(part, 1);
  if (threadIdx.x != 0) return;
  st->count = (unsigned)cnt;
  st->mse = cnt > 0 ? d2 / cnt : 0.0;
  st->inner_steps = 0;
  if (cnt < 4.0) {
    st->inner_done = 1;
    st->converged = 0;
    st->reason = GHICP_ICP_NO_CORRESPONDENCES;
    return;
  }
  st->inner_done = 0;
  const float* T = st->T;
  st->x[0] = (double)T[3]; st->x[1] = (double)T[7]; st->x[2] = (double)T[11];
  st->x[3] = atan2((double)T[9], (double)T[10]);
  st->x[4] = asin(fmin(1.0, fmax(-1.0, -(double)T[8])));
  st->x[5] = atan2((double)T[4], (double)T[0]);
  gicp_state_rot(st);
}

// one Gauss-Newton step's sums over the correspondences: J^T M J (21, upper triangle row by row), J^T M r (6), r^T M r (1);
// r = R(x) s + t(x) - t_j and J = [I | dR/droll s, dR/dpitch s, dR/dyaw s], all f64
__device__ inline void gicp_acc_body(const float4* __restrict__ src, const float4* __restrict__ tgt, const int* __restrict__ nn, int ns,
                                     const double* __restrict__ mahal, const GicpState* __restrict__ st, double* __restrict__ part, unsigned blk) {
  if (st->inner_done) return;
  __shared__ double red[16];
  double R[9], dR[27], x[6];
  for (int e = 0; e < 9; e++) R[e] = st->R[e];
  for (int e = 0; e < 27; e++) dR[e] = st->dR[e];
  for (int e = 0; e < 6; e++) x[e] = st->x[e];
  double acc[28];
#pragma unroll
  for (int d = 0; d < 28; d++) acc[d] = 0;
  for (unsigned i = blk * 256u + threadIdx.x; i < (unsigned)ns; i += NBLK * 256u) {
    const int j = nn[i];
    if (j < 0) continue;
    const float4 S = src[i], D = tgt[j];
    const double s[3] = {(double)S.x, (double)S.y, (double)S.z};
    double r[3], J[3][6];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      r[q] = (((R[q * 3] * s[0] + R[q * 3 + 1] * s[1]) + R[q * 3 + 2] * s[2]) + x[q]) - (q == 0 ? (double)D.x : (q == 1 ? (double)D.y : (double)D.z));
#pragma unroll
      for (int p = 0; p < 3; p++) J[q][p] = q == p ? 1.0 : 0.0;
#pragma unroll
      for (int a = 0; a < 3; a++) J[q][3 + a] = (dR[a * 9 + q * 3] * s[0] + dR[a * 9 + q * 3 + 1] * s[1]) + dR[a * 9 + q * 3 + 2] * s[2];
    }
    const double* m = &mahal[(size_t)i * 6];
    const double M[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
    double Mr[3], MJ[3][6];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      Mr[q] = (M[q * 3] * r[0] + M[q * 3 + 1] * r[1]) + M[q * 3 + 2] * r[2];
#pragma unroll
      for (int p = 0; p < 6; p++) MJ[q][p] = (M[q * 3] * J[0][p] + M[q * 3 + 1] * J[1][p]) + M[q * 3 + 2] * J[2][p];
    }
    int k = 0;
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
      for (int q = p; q < 6; q++) acc[k++] += (J[0][p] * MJ[0][q] + J[1][p] * MJ[1][q]) + J[2][p] * MJ[2][q];
#pragma unroll
    for (int p = 0; p < 6; p++) acc[21 + p] += (J[0][p] * Mr[0] + J[1][p] * Mr[1]) + J[2][p] * Mr[2];
    acc[27] += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
  }
  store_partials(acc, 28, red, part, blk);
}

// the step: partials reduced in wave_reduce_partials order, each group (H, g, e) rounded by N2, H dx = -g by elimination with partial
// pivoting, x += dx; a singular or non-finite solve stops the inner loop without a step
__device__ inline void gicp_solve_body(GicpState* st, const double* __restrict__ part) {
  if (st->inner_done) return;
  double acc[28];
  for (int d = 0; d < 28; d++) acc[d] = wave_reduce_partials(part, d);
  if (threadIdx.x != 0) return;
  gh_quant_grid(acc, 21);
  gh_quant_grid(acc + 21, 6);
  double A[6][6], bb[6], dx[6];
  int k = 0;
  for (int r = 0; r < 6; r++)
    for (int q = r; q < 6; q++) { A[r][q] = acc[k]; A[q][r] = acc[k]; k++; }
  for (int r = 0; r < 6; r++) bb[r] = -acc[21 + r];
  for (int c = 0; c < 6; c++) {
    int piv = c;
    for (int r = c + 1; r < 6; r++) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
    if (piv != c) {
      for (int q = 0; q < 6; q++) { const double t = A[c][q]; A[c][q] = A[piv][q]; A[piv][q] = t; }
      const double t = bb[c]; bb[c] = bb[piv]; bb[piv] = t;
    }
    for (int r = c + 1; r < 6; r++) {
      const double f = A[r][c] / A[c][c];
      for (int q = c; q < 6; q++) A[r][q] -= f * A[c][q];
      bb[r] -= f * bb[c];
    }
  }
  double mx = 0;
  for (int r = 5; r >= 0; r--) {
    double s = bb[r];
    for (int q = r + 1; q < 6; q++) s -= A[r][q] * dx[q];
    dx[r] = s / A[r][r];
    mx = fmax(mx, fabs(dx[r]));
  }
  st->inner_steps++;
  if (!(mx <= 1e300)) { st->inner_done = 1; return; }  // singular / non-finite: no step
  for (int p = 0; p < 6; p++) st->x[p] += dx[p];
  gicp_state_rot(st);
  if (mx < kGicpStop) st->inner_done = 1;
}

// applyState in float (the f64 closed form of R(x) rounded entry by entry), then the delta test of GICP's computeTransformation
__device__ inline void gicp_outer_body(GicpState* st) {
  if (st->reason == GHICP_ICP_NO_CORRESPONDENCES) return;
  float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)st->R[r * 3 + c];
    T[r * 4 + 3] = (float)st->x[r];
  }
  double delta = 0;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      const double ratio = (r < 3 && c < 3) ? st->inv_eps_r : st->inv_eps_t;
      const double cd = ratio * fabs((double)st->T[r * 4 + c] - (double)T[r * 4 + c]);
      if (cd > delta) delta = cd;
    }
  for (int d = 0; d < 16; d++) st->T[d] = T[d];
  st->iterations++;
  if (st->iterations >= st->max_iter) { st->converged = 1; st->reason = GHICP_ICP_ITERATIONS; }
  else if (delta < 1.0) { st->converged = 1; st->reason = GHICP_ICP_TRANSFORM; }
}

}  // namespace icpdev

// the fine + coarse grids ghicp_icp searches over a target, built in the context's grid buffers (icp.hip) with the cell chosen from the data
int gh_icp_build_index(ghicp_ctx* ctx, const float* xyz, long long n, int stride, icpdev::NnIndex* out);
