// Internal: what the per-stage kernels of the GH-ICP loop (loop.hip) and the persistent pair loop (pair_loop.hip) share -- the per-pair descriptor
// and state, the combined-distance evaluator, and the bodies of the stages (by block coordinates of the stand-alone kernel: the same sums).
#pragma once
#include "ctx.h"
#include "devmath.h"

#include <cmath>

#include "km_prob.h"

struct LoopState {
  int it, done, cor, converged_flag;
  double RMS, FDM, FDstd, IoU, para1, para2, penalty, CDmean, CDstd, energy;
  double Rt_till[16];
  double rmse_after;
  unsigned long long t_begin, t_end;  // persistent pair loop: when a slot took the pair and when it let go (s_memrealtime, 100 MHz)
  // diagnostics of the persistent loop (kernel timing on; round 6, the stragglers of DESIGN.md §6): the pair's longest Kuhn-Munkres solve, the
  // iteration it belongs to, and where the slot ran (HW_ID: compute unit / shader array / engine, XCC_ID: the die)
  unsigned long long t_solve_max;
  int it_solve_max;
  unsigned hw_id;
};

struct LoopConst {
  int ks, kt, n, feature, corr, max_iter, min_cor, nchunk_a, nchunk_b, chunk_a, chunk_b, nparts;
  float scale, est_iou, adjust_ratio, adjust_step;
  double converge_t, converge_r, penalty_initial, km_eps;
};

// one registration job of the batch; every pointer is device memory
struct LoopProb {
  LoopConst C;
  LoopState* st;
  double* kpS;            // the pair's own copy (the loop transforms it in place)
  const double* kpS_src;  // where it is copied from when the batch starts
  const double* kpT;
  const void* FD;   // [ks][kt]
  const void* FDt;  // [kt][ks]
  int fdt_given;    // the job came with its transposed matrix (k_pairs_transpose skips it)
  const double* wfd;
  double *pminA, *pminB, *psum;
  int *pidxA, *pidxB, *SP, *TP, *SVs, *TVs;
  ghicp_iter* trace;
  int* matchlist;
  int ml_row0;  // matchlist row of iteration `it` is it - ml_row0 (a resumed loop hands over one row per call)
  // KM
  unsigned *km_cnt, *km_rptr;
  int *km_cols, *kmmatch, *km_status;
  double *km_vals, *km_lx, *kmw;
  Km2Problem* km_desc;
};

constexpr int ROWS = 256;       // threads per block in the sweep = rows handled per block
constexpr int CHUNK_MAX = 512;  // columns staged in LDS per block

// pair_loop.hip: a Kuhn-Munkres batch whose every graph fits the LDS-resident solver, classes and order as planned, until every pair is done
template <int FT> int run_pair_loop(ghicp_ctx* ctx, const LoopProb* dprobs, int nb, const Km4Plan& plan, int* dqheads);

// The combined distance CD(i, j) of one iteration, the ONLY spelling of it: every stage builds one of these from (P, it), so the sweep, the graph's
// count and fill, the fused stages and the dense weights see the same bits (-ffp-contract=off: the bits follow from the text).  f: the feature
// distance in its own type; the feature NONE reads none.
template <int FT> struct FdType { typedef uint16_t T; };
template <> struct FdType<GHICP_FEATURE_FPFH> { typedef float T; };

template <int FT>
struct CdEval {
  typedef typename FdType<FT>::T fd_t;
  double wed = 1, wfd = 0, inv_k, scale;
  __device__ CdEval(const LoopProb& P, const int it) : inv_k(1.0 / (double)(it + 1)), scale((double)P.C.scale) {
    if (FT == GHICP_FEATURE_BSC) { wfd = P.wfd[it]; wed = 1.0 - wfd; }
  }
  __device__ double ed(double ax, double ay, double az, double bx, double by, double bz) const {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return scale * sqrt(dx * dx + dy * dy + dz * dz);  // ghicp_reg.cpp:122
  }
  __device__ double cd(double ed, fd_t f) const {
    if (FT == GHICP_FEATURE_BSC) return wed * ed + wfd * (double)f;        // ghicp_reg.cpp:259
    if (FT == GHICP_FEATURE_FPFH) return 1.0 * ed / pow((double)f, inv_k);  // ghicp_reg.cpp:308
    return ed;                                                              // ghicp_reg.cpp:224
  }
  // a feature matrix as its own type, and element idx of it
  __device__ static const fd_t* typed(const void* F) { return reinterpret_cast<const fd_t*>(F); }
  __device__ static fd_t at(const fd_t* F, size_t idx) { return FT != GHICP_FEATURE_NONE ? F[idx] : (fd_t)0; }
  // CD of keypoint pair (0, 0): the pivot of the sums
  __device__ double pivot(const LoopProb& P) const { return cd(ed(P.kpS[0], P.kpS[1], P.kpS[2], P.kpT[0], P.kpT[1], P.kpT[2]), at(typed(P.FD), 0)); }
};

namespace {

// One sweep: thread = "row" a (keypoint of set A), loop over a chunk of set B staged in LDS.
// The feature matrix is read as [b][a] so that lanes (consecutive a) touch consecutive addresses.
// Row arg-min semantics = ghicp_reg.cpp:715-724 / 622-650: start (9e20, 0), strict '<', ascending index.
// (bx, by) = the block coordinates of the stand-alone kernel; sB: CHUNK_MAX * 3 doubles, red: 16 doubles of LDS.  The persistent
// pair loop calls the same body for every (bx, by) in turn, so both paths produce the same partial sums in the same order.
template <int FT, bool COLS>
__device__ inline void dev_cd_rowmin(const LoopProb& P, const int bx, const int by, double* sB, double* red) {
  const int ka = COLS ? P.C.kt : P.C.ks, kb = COLS ? P.C.ks : P.C.kt;
  const int chunk = COLS ? P.C.chunk_a : P.C.chunk_b, nchunk = COLS ? P.C.nchunk_a : P.C.nchunk_b;
  if (by >= nchunk || bx * ROWS >= ka) return;
  const double* A = COLS ? P.kpT : P.kpS;
  const double* B = COLS ? P.kpS : P.kpT;
  const CdEval<FT> E(P, P.st->it);
  const typename CdEval<FT>::fd_t* F = E.typed(COLS ? P.FD : P.FDt);
  const int jb = by * chunk;
  const int je = min(kb, jb + chunk);
  for (int t = threadIdx.x; t < (je - jb) * 3; t += ROWS) sB[t] = B[(size_t)jb * 3 + t];
  __syncthreads();
  const int a = bx * ROWS + threadIdx.x;
  const bool live = a < ka;
  double ax = 0, ay = 0, az = 0;
  if (live) { ax = A[(size_t)a * 3]; ay = A[(size_t)a * 3 + 1]; az = A[(size_t)a * 3 + 2]; }
  double best = 9e20, s = 0, s2 = 0;
  int bidx = 0;
  // CDmean / CDstd are accumulated around a pivot (the CD of keypoint pair (0,0), the same value in every block and in
  // k_penalty): sum^2 / n - mean^2 would cancel when the spread of CD is small against its mean (ghicp_reg.cpp:266-273 is two-pass)
  double piv = 0;
  if (!COLS) piv = E.pivot(P);
  if (live) {
    for (int j = jb; j < je; j++) {
      const double cd = E.cd(E.ed(ax, ay, az, sB[(j - jb) * 3], sB[(j - jb) * 3 + 1], sB[(j - jb) * 3 + 2]), E.at(F, (size_t)j * ka + a));
      if (cd < best) { best = cd; bidx = j; }
      if (!COLS) { const double c0 = cd - piv; s += c0; s2 += c0 * c0; }
    }
    (COLS ? P.pminB : P.pminA)[(size_t)by * ka + a] = best;
    (COLS ? P.pidxB : P.pidxA)[(size_t)by * ka + a] = bidx;
  }
  if (!COLS) {
    const double bs = gh_block_sum(s, red);
    const double bs2 = gh_block_sum(s2, red);
    if (threadIdx.x == 0) {
      const size_t b = (size_t)by * cdiv_dev(ka, ROWS) + bx;
      P.psum[b * 2] = bs;
      P.psum[b * 2 + 1] = bs2;
    }
  }
}

// The penalty of iterations 2, 3, ... of the BSC and FPFH energies (ghicp_reg.cpp:274-283, 326-331): from the state the PREVIOUS iteration
// left, not from this iteration's sweep.  One function for dev_penalty and for the persistent loop's fused sweep, which needs the value
// before the sums exist: the same expression, the same bits.
__device__ inline double gh_penalty_from_state(const LoopState* st, const LoopConst& C, const double* wfdtab, const int it) {
  if (C.feature == GHICP_FEATURE_BSC) {
    const double wfd = wfdtab[it], wed = 1.0 - wfd;
    return fmax(st->RMS * st->para1 * (double)C.scale * wed + (st->FDM + st->para2 * st->FDstd) * wfd, 5.0);
  }
  return st->RMS * st->para1 * (double)C.scale * st->para2;
}

// calCD_* tails: CDmean, CDstd, penalty (ghicp_reg.cpp:228-239, 264-287, 317-335)
__device__ inline void dev_penalty(const LoopProb& P, double* red) {
  LoopState* st = P.st;
  const LoopConst& C = P.C;
  double s = 0, s2 = 0;
  for (int i = threadIdx.x; i < C.nparts; i += blockDim.x) { s += P.psum[i * 2]; s2 += P.psum[i * 2 + 1]; }
  s = gh_block_sum(s, red);
  s2 = gh_block_sum(s2, red);
  if (threadIdx.x == 0) {
    const int it = st->it;
    const double cnt = (double)C.ks * (double)C.kt;
    double piv;
    if (C.feature == GHICP_FEATURE_BSC) piv = CdEval<GHICP_FEATURE_BSC>(P, it).pivot(P);
    else if (C.feature == GHICP_FEATURE_FPFH) piv = CdEval<GHICP_FEATURE_FPFH>(P, it).pivot(P);
    else piv = CdEval<GHICP_FEATURE_NONE>(P, it).pivot(P);
    const double dm = s / (double)C.kt / (double)C.ks;  // mean of (CD - pivot)
    const double mean = piv + dm;
    double var = s2 / cnt - dm * dm;
    if (var < 0) var = 0;
    const double sd = sqrt(var);
    double pen;
    if (C.feature == GHICP_FEATURE_NONE) {
      pen = fmax(mean, 1.0);  // Q6: line 239 overrides 230-237
      st->CDstd = 0;
    } else if (C.feature == GHICP_FEATURE_BSC) {
      if (it > 1) pen = gh_penalty_from_state(st, C, P.wfd, it);
      else pen = fmax(mean - C.penalty_initial * sd, 5.0);
      st->CDstd = sd;
    } else {
      if (it > 1) pen = gh_penalty_from_state(st, C, P.wfd, it);
      else pen = mean / C.penalty_initial;
      st->CDstd = 0;
    }
    st->CDmean = mean;
    st->penalty = pen;
  }
}

// Sparse KM input (km_prob.h): per row the explicit entries (j, -CD) with CD < penalty (ghicp_reg.cpp:358-365);
// every other entry of the n x n graph is the background -penalty.  One wave per row over 64-column blocks, two passes (count, fill); tB: the
// target keypoints (P.kpT, or the persistent loop's copy in LDS).  MASK: the fused stages of pair_loop.hip keep a row's membership as a bitmask
// -- the count pass stores its ballots there, the fill reads them.  Count of row i < n: entries and row maximum (km.cpp:56-62; entries > -penalty)
template <int FT, bool MASK>
__device__ inline void dev_km_row_count(const LoopProb& P, const CdEval<FT>& E, const double* tB, const double pen, const int i, unsigned* mask) {
  const LoopConst& C = P.C;
  const int lane = threadIdx.x & 63;
  if (i >= C.ks) {  // padding rows: all background
    if (lane == 0) { P.km_cnt[i] = 0u; P.km_lx[i] = -pen; }
    return;
  }
  const typename CdEval<FT>::fd_t* F = E.typed(P.FD);
  const double sx = P.kpS[(size_t)i * 3], sy = P.kpS[(size_t)i * 3 + 1], sz = P.kpS[(size_t)i * 3 + 2];
  unsigned c = 0;
  double mx = -pen;
  for (int j0 = 0; j0 < C.kt; j0 += 64) {
    const int j = j0 + lane;
    bool e = false;
    if (j < C.kt) {
      const double cd = E.cd(E.ed(sx, sy, sz, tB[(size_t)j * 3], tB[(size_t)j * 3 + 1], tB[(size_t)j * 3 + 2]), E.at(F, (size_t)i * C.kt + j));
      e = cd < pen;
      if (e) mx = fmax(mx, -cd);
    }
    const unsigned long long b = __ballot(e);
    if (MASK && lane == 0) {
      mask[(size_t)(j0 >> 5) * C.ks + i] = (unsigned)b;
      mask[(size_t)((j0 >> 5) + 1) * C.ks + i] = (unsigned)(b >> 32);
    }
    c += __popcll(b);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) { P.km_cnt[i] = c; P.km_lx[i] = mx; }
}

// The fill of row i < ks: entry (j, -CD) at km_rptr[i] + its rank among the row's members.  MASK: the members come from the row's mask words (the
// next word is loaded before this one's block is worked on; a block without a member is skipped unread).  A row's entries equal its count by construction;
// even so the masked fill stores nothing at or beyond km_rptr[i + 1] and reports a mismatch in km_status (bit 8: the host fails the call)
template <int FT, bool MASK>
__device__ inline void dev_km_row_fill(const LoopProb& P, const CdEval<FT>& E, const double* tB, const double pen, const int i, const unsigned* mask) {
  const LoopConst& C = P.C;
  const int lane = threadIdx.x & 63;
  const typename CdEval<FT>::fd_t* F = E.typed(P.FD);
  int* __restrict__ cols = P.km_cols;
  double* __restrict__ vals = P.km_vals;
  const int nw = cdiv_dev(C.kt, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
  const double sx = P.kpS[(size_t)i * 3], sy = P.kpS[(size_t)i * 3 + 1], sz = P.kpS[(size_t)i * 3 + 2];
  const unsigned base = P.km_rptr[i], end = MASK ? P.km_rptr[i + 1] : 0u;
  unsigned c = 0;
  bool bad = false;
  unsigned long long next = MASK ? (unsigned long long)mask[i] | ((unsigned long long)mask[(size_t)C.ks + i] << 32) : 0ull;
  for (int w = 0; w < nw; w++) {
    const int j = w * 64 + lane;
    unsigned long long b = next;
    bool e;
    double cd = 0;
    if (MASK) {
      if (w + 1 < nw) next = (unsigned long long)mask[(size_t)(2 * w + 2) * C.ks + i] | ((unsigned long long)mask[(size_t)(2 * w + 3) * C.ks + i] << 32);
      if (b == 0ull) continue;
      e = (b >> lane) & 1ull;
    } else {
      e = j < C.kt;
    }
    if (e) cd = E.cd(E.ed(sx, sy, sz, tB[(size_t)j * 3], tB[(size_t)j * 3 + 1], tB[(size_t)j * 3 + 2]), E.at(F, (size_t)i * C.kt + j));
    if (!MASK) { e = e && cd < pen; b = __ballot(e); }
    if (e) {
      const unsigned off = base + c + __popcll(b & below);
      if (!MASK || off < end) { cols[off] = j; vals[off] = -cd; }
      else bad = true;
    }
    c += __popcll(b);
  }
  if (MASK && (bad || c != end - base)) atomicOr(P.km_status, 0x100);
}

// the stand-alone form: workgroup bx takes rows 4 bx .. 4 bx + 3, membership by comparison (FILL = 0: count, 1: fill)
template <int FT, int FILL>
__device__ inline void dev_km_csr(const LoopProb& P, const int bx) {
  const int i = bx * 4 + (int)(threadIdx.x >> 6);
  if (i >= P.C.n) return;
  const CdEval<FT> E(P, P.st->it);
  if (!FILL) dev_km_row_count<FT, false>(P, E, P.kpT, P.st->penalty, i, nullptr);
  else if (i < P.C.ks) dev_km_row_fill<FT, false>(P, E, P.kpT, P.st->penalty, i, nullptr);
}

// exclusive scan of the row counts (one block per pair) + the km2 problem descriptor
__device__ inline void dev_km_scan_desc(const LoopProb& P, int* sc) {
  const int n = P.C.n;
  int carry = 0;
  for (int base = 0; base < n; base += (int)blockDim.x) {
    const int i = base + threadIdx.x;
    const int v = i < n ? (int)P.km_cnt[i] : 0;
    int tot;
    const int ex = gh_block_excl_scan(v, sc, &tot);
    if (i < n) P.km_rptr[i] = (unsigned)(carry + ex);
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    P.km_rptr[n] = (unsigned)carry;
    Km2Problem p;
    p.n = n; p.pad_ = 0; p.bg = -P.st->penalty; p.eps = P.C.km_eps; p.row_ptr = P.km_rptr; p.cols = P.km_cols; p.vals = P.km_vals;
    p.lx_init = P.km_lx; p.match_out = P.kmmatch; p.status = P.km_status; p.done = &P.st->done; p.steps = nullptr;
    *P.km_desc = p;
  }
}

// Everything after the sweep, one 1024-thread workgroup per pair.
// red: 16 doubles, ired: 17 ints, sh: 32 doubles of LDS
template <int FT>
__device__ inline void dev_solve(const LoopProb& P, double* red, int* ired, double* sh) {
  LoopState* st = P.st;
  const LoopConst& C = P.C;
  double* kpS = P.kpS;
  const double* kpT = P.kpT;
  const typename CdEval<FT>::fd_t* FD = CdEval<FT>::typed(P.FD);
  int* SP = P.SP;
  int* TP = P.TP;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int it = st->it;
  const double penalty = st->penalty;
  int* matchlist = P.matchlist;
  if (matchlist)
    for (int i = tid; i < C.ks; i += nt) matchlist[(size_t)(it - P.ml_row0) * C.ks + i] = -1;

  // ---- correspondences, in the reference's emission order
  int cor = 0;
  if (C.corr == GHICP_CORR_KM) {
    // Km::output (km.cpp:157-171): ascending y, kept iff w[match[y]][y] != -penalty (exact compare)
    double e = 0;
    for (int base = 0; base < C.n; base += nt) {
      const int y = base + tid;
      int flag = 0, x = -1;
      if (y < C.n) x = P.kmmatch[y];
      if (y < C.n && x >= 0) {  // x < 0: the solver gave up (non-finite weights); no correspondence, status reported by the host
        double g = -penalty;
        if (P.km_rptr) {  // sparse graph: (x,y) carries a weight != -penalty iff it is an explicit entry
          unsigned lo = P.km_rptr[x], hi = P.km_rptr[x + 1];
          const unsigned end = hi;
          while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (P.km_cols[mid] < y) lo = mid + 1; else hi = mid; }
          if (lo < end && P.km_cols[lo] == y) g = P.km_vals[lo];
        } else {
          g = P.kmw[(size_t)x * C.n + y];
        }
        flag = (g != -penalty) ? 1 : 0;
        if (g != -10000.0) e -= g;  // Calenergy (km.cpp:128-141): INF = 10000 never matches
      }
      int tot;
      const int pos = gh_block_excl_scan(flag, ired, &tot);
      if (flag) { SP[cor + pos] = x; TP[cor + pos] = y; }
      cor += tot;
      __syncthreads();
    }
    e = gh_block_sum(e, red);
    if (tid == 0) st->energy = e;
  } else {
    // row arg-min over chunks (ascending chunk == ascending column)
    for (int i = tid; i < C.ks; i += nt) {
      double best = 9e20; int bi = 0;
      for (int c = 0; c < C.nchunk_b; c++) {
        const double v = P.pminA[(size_t)c * C.ks + i];
        if (v < best) { best = v; bi = P.pidxA[(size_t)c * C.ks + i]; }
      }
      P.SVs[i] = bi;
      P.TVs[C.kt + i] = (best < penalty) ? 1 : 0;  // NN acceptance flag (ghicp_reg.cpp:725)
    }
    if (C.corr == GHICP_CORR_NNR) {
      for (int j = tid; j < C.kt; j += nt) {
        double best = 9e20; int bi = 0;
        for (int c = 0; c < C.nchunk_a; c++) {
          const double v = P.pminB[(size_t)c * C.kt + j];
          if (v < best) { best = v; bi = P.pidxB[(size_t)c * C.kt + j]; }
        }
        P.TVs[j] = bi;
      }
    }
    __syncthreads();
    for (int base = 0; base < C.ks; base += nt) {
      const int i = base + tid;
      int flag = 0, sv = 0;
      if (i < C.ks) {
        sv = P.SVs[i];
        if (C.corr == GHICP_CORR_NN) flag = P.TVs[C.kt + i];
        else flag = (C.kt > 0 && P.TVs[sv] == i) ? 1 : 0;  // Q7: reciprocal test only (ghicp_reg.cpp:654)
      }
      int tot;
      const int pos = gh_block_excl_scan(flag, ired, &tot);
      if (flag) { SP[cor + pos] = i; TP[cor + pos] = sv; }
      cor += tot;
      __syncthreads();
    }
  }
  __syncthreads();
  if (matchlist)
    for (int c = tid; c < cor; c += nt) matchlist[(size_t)(it - P.ml_row0) * C.ks + SP[c]] = TP[c];

  // ---- RMSE, FDM, FDstd (ghicp_reg.cpp:548-578)
  double rm = 0, fm = 0;
  for (int c = tid; c < cor; c += nt) {
    const int i = SP[c], j = TP[c];
    const double dx = kpS[(size_t)i * 3] - kpT[(size_t)j * 3], dy = kpS[(size_t)i * 3 + 1] - kpT[(size_t)j * 3 + 1],
                 dz = kpS[(size_t)i * 3 + 2] - kpT[(size_t)j * 3 + 2];
    rm += dx * dx + dy * dy + dz * dz;
    if (FT != GHICP_FEATURE_NONE) fm += (double)FD[(size_t)i * C.kt + j];
  }
  rm = gh_block_sum(rm, red);
  fm = gh_block_sum(fm, red);
  const double FDM = fm / (double)cor;
  double fc = 0;
  if (FT != GHICP_FEATURE_NONE)
    for (int c = tid; c < cor; c += nt) {
      const int i = SP[c], j = TP[c];
      double f = (double)FD[(size_t)i * C.kt + j];
      f -= FDM;
      fc += f * f;
    }
  fc = gh_block_sum(fc, red);
  const double FDstd = sqrt(fc / (double)cor);
  const double RMSE = sqrt(rm / (double)cor);

  // ---- float Umeyama (ghicp_reg.cpp:839-866): inputs cast to f32, means/cross-covariance in f64, matrix rounded once (N2)
  double m[6] = {0, 0, 0, 0, 0, 0};
  for (int c = tid; c < cor; c += nt) {
    const int i = SP[c], j = TP[c];
    for (int d = 0; d < 3; d++) { m[d] += (double)(float)kpS[(size_t)i * 3 + d]; m[3 + d] += (double)(float)kpT[(size_t)j * 3 + d]; }
  }
  for (int d = 0; d < 6; d++) m[d] = gh_block_sum(m[d], red);
  float msf[3], mtf[3];
  for (int d = 0; d < 3; d++) { msf[d] = (float)(m[d] / (double)cor); mtf[d] = (float)(m[3 + d] / (double)cor); }
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = tid; c < cor; c += nt) {
    const int i = SP[c], j = TP[c];
    double a[3], b[3];
    for (int d = 0; d < 3; d++) {
      a[d] = (double)(float)kpT[(size_t)j * 3 + d] - (double)mtf[d];
      b[d] = (double)(float)kpS[(size_t)i * 3 + d] - (double)msf[d];
    }
    for (int r = 0; r < 3; r++)
      for (int q = 0; q < 3; q++) H[r * 3 + q] += a[r] * b[q];
  }
  for (int d = 0; d < 9; d++) H[d] = gh_block_sum(H[d], red);
  if (tid == 0) {
    double A[9], R[9];
    for (int d = 0; d < 9; d++) A[d] = H[d] / (double)cor;
    gh_quant_grid(A, 9);  // N2: umeyama's sigma is a Matrix3f
    gh_kabsch(A, R);
    float Rf[9], tf[3];
    for (int d = 0; d < 9; d++) Rf[d] = (float)R[d];
    for (int r = 0; r < 3; r++)
      tf[r] = (float)((double)mtf[r] -
                      (((double)Rf[r * 3] * (double)msf[0] + (double)Rf[r * 3 + 1] * (double)msf[1]) + (double)Rf[r * 3 + 2] * (double)msf[2]));
    for (int r = 0; r < 3; r++) {
      for (int q = 0; q < 3; q++) sh[r * 4 + q] = (double)Rf[r * 3 + q];
      sh[r * 4 + 3] = (double)tf[r];
    }
  }
  __syncthreads();
  double Rt[12];
  for (int d = 0; d < 12; d++) Rt[d] = sh[d];

  // ---- RMSE after (on the correspondences, before kpS is overwritten) and update of ALL source keypoints
  double ra = 0;
  for (int c = tid; c < cor; c += nt) {
    const int i = SP[c], j = TP[c];
    const double x = kpS[(size_t)i * 3], y = kpS[(size_t)i * 3 + 1], z = kpS[(size_t)i * 3 + 2];
    const double nx = ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[3];
    const double ny = ((Rt[4] * x + Rt[5] * y) + Rt[6] * z) + Rt[7];
    const double nz = ((Rt[8] * x + Rt[9] * y) + Rt[10] * z) + Rt[11];
    const double dx = nx - kpT[(size_t)j * 3], dy = ny - kpT[(size_t)j * 3 + 1], dz = nz - kpT[(size_t)j * 3 + 2];
    ra += dx * dx + dy * dy + dz * dz;
  }
  ra = gh_block_sum(ra, red);
  __syncthreads();
  for (int i = tid; i < C.ks; i += nt) {
    const double x = kpS[(size_t)i * 3], y = kpS[(size_t)i * 3 + 1], z = kpS[(size_t)i * 3 + 2];
    kpS[(size_t)i * 3] = ((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[3];
    kpS[(size_t)i * 3 + 1] = ((Rt[4] * x + Rt[5] * y) + Rt[6] * z) + Rt[7];
    kpS[(size_t)i * 3 + 2] = ((Rt[8] * x + Rt[9] * y) + Rt[10] * z) + Rt[11];
  }

  if (tid == 0) {
    const double RMSEafter = sqrt(ra / (double)cor);
    bool conv = false;
    if (cor < C.min_cor) conv = true;  // ghicp_reg.cpp:796
    const double IoU = 1.0 * (double)cor / (double)(C.ks + C.kt - cor);
    const double dx = Rt[3], dy = Rt[7], dz = Rt[11];
    double ax = atan2(Rt[9], Rt[10]);
    double ay = atan2(-Rt[8], sqrt(Rt[9] * Rt[9] + Rt[10] * Rt[10]));
    double az = atan2(Rt[1], Rt[0]);
    const double pi = 3.1415926;
    ax = ax / pi * 180; ay = ay / pi * 180; az = az / pi * 180;
    if (fabs(dx) < C.converge_t && fabs(dy) < C.converge_t && fabs(dz) < C.converge_t && fabs(ax) < C.converge_r &&
        fabs(ay) < C.converge_r && fabs(az) < C.converge_r)
      conv = true;
    double p1 = st->para1, p2 = st->para2;  // adjustweight ghicp_reg.cpp:771-789
    if ((double)C.est_iou / IoU > (double)C.adjust_ratio) { p1 += (double)C.adjust_step; p2 += (double)C.adjust_step; }
    else if (IoU / (double)C.est_iou > (double)C.adjust_ratio) { p1 -= (double)C.adjust_step; p2 -= (double)C.adjust_step; }
    double nt16[16];
    const double Rt16[16] = {Rt[0], Rt[1], Rt[2], Rt[3], Rt[4], Rt[5], Rt[6], Rt[7], Rt[8], Rt[9], Rt[10], Rt[11], 0, 0, 0, 1};
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) {
        double s = 0;
        for (int k = 0; k < 4; k++) s += Rt16[r * 4 + k] * st->Rt_till[k * 4 + c];
        nt16[r * 4 + c] = s;
      }
    for (int d = 0; d < 16; d++) st->Rt_till[d] = nt16[d];
    ghicp_iter rec;
    rec.cor = cor; rec.converged = conv ? 1 : 0;
    rec.penalty = penalty; rec.cdmean = st->CDmean; rec.cdstd = st->CDstd; rec.rmse = RMSE; rec.rmse_after = RMSEafter;
    rec.fdm = FDM; rec.fdstd = FDstd; rec.iou = IoU; rec.para1 = p1; rec.para2 = p2;
    rec.energy = (C.corr == GHICP_CORR_KM) ? st->energy : 0.0;
    for (int d = 0; d < 16; d++) rec.Rt[d] = Rt16[d];
    P.trace[it] = rec;
    st->RMS = RMSE; st->FDM = FDM; st->FDstd = FDstd; st->IoU = IoU; st->para1 = p1; st->para2 = p2; st->cor = cor;
    st->rmse_after = RMSEafter;
    st->it = it + 1;
    if (conv || it + 1 >= C.max_iter) { st->done = 1; st->converged_flag = conv ? 1 : 0; }
  }
}

}  // namespace
